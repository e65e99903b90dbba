"""CPU: the reference's example_configs/speech2text/lstm_small_1gpu.py — 13 psf MFCCs straight into a two-layer
unidirectional cudnn_lstm, no convolution — loads UNCHANGED, its data-layer parameters pass check_params and
select the psf-MFCC front end; all six (backend, input_type) combinations of the reference dispatch explicitly."""
import os

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = "/root/reference/example_configs/speech2text/lstm_small_1gpu.py"
needs_ref = pytest.mark.skipif(not os.path.exists(CFG), reason="reference checkout not present")


@needs_ref
def test_lstm_small_config_selects_the_psf_mfcc_front_end(monkeypatch):
  monkeypatch.chdir(REPO)               # the config names the toy vocabulary relative to the repository root
  from openseq2seq_amd.data.speech2text import speech_utils as su
  from openseq2seq_amd.data.speech2text.speech2text import Speech2TextDataLayer
  from openseq2seq_amd.encoders.ds2_encoder import DeepSpeech2Encoder
  from openseq2seq_amd.models.speech2text import Speech2Text
  from openseq2seq_amd.utils.utils import get_base_config
  _, base, model_cls, mod = get_base_config(["--config_file=" + CFG, "--mode=train"])
  assert model_cls is Speech2Text and base["encoder"] is DeepSpeech2Encoder
  enc = base["encoder_params"]
  assert enc["conv_layers"] == [] and enc["rnn_type"] == "cudnn_lstm" and enc["rnn_unidirectional"] is True
  DeepSpeech2Encoder(enc, None, mode="train")                               # schema accepted
  for key in ("train_params", "eval_params"):
    p = dict(mod[key]["data_layer_params"], mode="train" if key == "train_params" else "eval", batch_size=2)
    assert p["input_type"] == "mfcc" and p["num_audio_features"] == 13 and p.get("backend", "psf") == "psf"
    dl = Speech2TextDataLayer(p, None, 1, 0)                                # check_params passes
    assert su.front_end_class(dl.params) is su.PsfMfccFrontEnd
    assert dl._psf()                    # augmentation on the raw samples, framesig's frame count
    assert dl.frames_for_samples(320) == 1 and dl.frames_for_samples(321) == 2 and dl.frames_for_samples(16000) == 99
    fe = su.make_front_end(dl.params, torch.device("cpu"))                  # tables only: no kernel runs
    assert isinstance(fe, su.PsfMfccFrontEnd) and tuple(fe.fb.shape) == (26, 257) and tuple(fe.dctl.shape) == (13, 26)
    assert fe.frames(16000) == 104 and fe.frames(319) == 8
  assert "time_stretch_ratio" in mod["train_params"]["data_layer_params"]["augmentation"]


def test_every_reference_combination_dispatches():
  from openseq2seq_amd.data.speech2text import speech_utils as su
  want = {("psf", "spectrogram"): su.PsfSpectrogramFrontEnd, ("psf", "logfbank"): su.PsfLogfbankFrontEnd,
          ("psf", "mfcc"): su.PsfMfccFrontEnd, ("librosa", "logfbank"): su.LogMelFrontEnd,
          ("librosa", "mfcc"): su.LibrosaMfccFrontEnd, ("librosa", "spectrogram"): su.LibrosaSpectrogramFrontEnd}
  for (backend, input_type), cls in want.items():
    assert su.front_end_class(dict(backend=backend, input_type=input_type)) is cls
  assert su.front_end_class(dict(input_type="mfcc")) is su.PsfMfccFrontEnd            # backend defaults to psf
  with pytest.raises(NotImplementedError, match=r"backend='psf'.*input_type='cepstrum'"):
    su.make_front_end(dict(input_type="cepstrum", num_audio_features=13), torch.device("cpu"))
