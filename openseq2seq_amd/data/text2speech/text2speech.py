"""Text2SpeechDataLayer — parameter schema and batch contract of
open_seq2seq/data/text2speech/text2speech.py:22-545.

Batch contract (train): source_tensors = [text ids int32 [B,S] (pad <p>=0, </s>=2),
text lengths [B]] (+ [style mel fp32 [B,T,n_mel], style lengths] with style_input "wav");
target_tensors = [spec fp32 [B,T,n_mel(+n_mag)], stop token fp32 [B,T], spec lengths [B]].
With output_type "both" the target is concat(log-mel, magnitude) and the magnitude is
exp(log_mag) when exp_mag (:486-488); pad_EOS appends frames carrying log(data_min) /
data_min and stop token 1 and the returned lengths include them (:494-545). The character
vocabulary is the file + 3 special symbols (:137-148). The csv/wav reading path is
host-side; feature extraction itself is the GPU kernel behind
data/text2speech/speech_utils.py. `synthetic_batch` draws SURVEY.md 8d's cfg-5 workload.
`get_magnitude_spec` (:656-715) turns a predicted spectrogram back into the magnitudes the Griffin-Lim export
of the infer mode reads (models/text2speech.py)."""
from __future__ import absolute_import, division, print_function

import io
import math

import numpy as np
import torch

from ..data_layer import DataLayer
from ..speech2text.speech_utils import mel_basis_slaney
from .speech_utils import denormalize, inverse_mel, mel_basis_htk


class Text2SpeechDataLayer(DataLayer):
  @staticmethod
  def get_required_params():
    return dict(DataLayer.get_required_params(), **{
        'dataset_location': str, 'dataset': ['LJ', 'MAILABS'], 'num_audio_features': None,
        'output_type': ['magnitude', 'mel', 'both'], 'vocab_file': str, 'dataset_files': list,
        'feature_normalize': bool,
    })

  @staticmethod
  def get_optional_params():
    return dict(DataLayer.get_optional_params(), **{
        'pad_to': int, 'mag_power': int, 'pad_EOS': bool, 'pad_value': float,
        'feature_normalize_mean': float, 'feature_normalize_std': float, 'trim': bool,
        'data_min': None, 'duration_min': int, 'duration_max': int,
        'mel_type': ['slaney', 'htk'], 'exp_mag': bool, 'style_input': [None, 'wav'],
        'n_samples_train': int, 'n_samples_eval': int, 'n_fft': int, 'fmax': float,
        'max_normalization': bool, 'use_cache': bool,
    })

  def __init__(self, params, model, num_workers=None, worker_id=None):
    super(Text2SpeechDataLayer, self).__init__(params, model, num_workers or 1, worker_id or 0)
    p = self.params
    chars = []
    try:
      with io.open(p['vocab_file'], "r", encoding="utf-8") as f:
        chars = [line.rstrip("\n") for line in f if line.rstrip("\n") != ""]
    except IOError:
      chars = [chr(32 + i) for i in range(91)]
    # ids start at 3: <p> = 0, <s> = 1, </s> = 2  (text2speech.py:137-148)
    p['char2idx'] = {c: i + 3 for i, c in enumerate(chars)}
    p['char2idx'].update({'<p>': 0, '<s>': 1, '</s>': 2})
    p['idx2char'] = {i: c for c, i in p['char2idx'].items()}
    p['src_vocab_size'] = len(p['char2idx'])
    self._both = p['output_type'] == "both"
    self._exp_mag = bool(p.get('exp_mag', False)) and self._both
    self._mel = "mel" in p['output_type']
    # text2speech.py:137-142: LJSpeech 22.05 kHz with n_fft 1024 unless set, M-AILABS 16 kHz with n_fft 800
    if p.get('dataset') == 'LJ':
      self._sampling_rate, self._n_fft = 22050, p.get('n_fft', 1024)
    else:
      self._sampling_rate, self._n_fft = 16000, 800
    self.max_normalization = p.get('max_normalization', False)
    self._mel_basis_cache = None

  def build_graph(self):
    return self

  @property
  def input_tensors(self):
    return {}

  @property
  def sampling_rate(self):
    return self._sampling_rate

  @property
  def n_fft(self):
    return self._n_fft

  @property
  def _mel_basis(self):
    """librosa.filters.mel of the configuration (text2speech.py:214-229), [n_mels, n_fft/2 + 1]; None for a
    magnitude-only layer. Built on first use."""
    if not (self._mel or self._both):
      return None
    if self._mel_basis_cache is None:
      n_mels = self.feature_sizes()[0]
      make = mel_basis_slaney if self.params.get('mel_type', 'htk') == 'slaney' else mel_basis_htk
      self._mel_basis_cache = make(self._sampling_rate, self._n_fft, n_mels, fmax=self.params.get('fmax', None))
    return self._mel_basis_cache

  def get_magnitude_spec(self, spectrogram, is_mel=False):
    """text2speech.py:656-715: the energy magnitude spectrogram [time, n_fft/2 + 1] of a model output
    [time, features]. A mel layer (or the mel half of a "both" layer, is_mel=True) goes through inverse_mel; a
    magnitude output is denormalised, padded with data_min up to n_fft/2 + 1 bins and scaled by 1 / mag_power
    (and exponentiated when the layer stores log magnitudes)."""
    p = self.params
    spectrogram = np.asarray(spectrogram).astype(float)
    mean, std = p.get("feature_normalize_mean", 0.), p.get("feature_normalize_std", 1.)
    if self._mel or (is_mel and self._both):
      slaney = p.get('mel_type', 'htk') == 'slaney'
      return inverse_mel(spectrogram, fs=self._sampling_rate, n_fft=self._n_fft, n_mels=self.feature_sizes()[0],
                         power=p.get('mag_power', 2), feature_normalize=p["feature_normalize"], mean=mean, std=std,
                         mel_basis=self._mel_basis, htk=not slaney, norm=1 if slaney else None)
    if p["feature_normalize"]:
      spectrogram = denormalize(spectrogram, mean, std)
    n_feats = p['num_audio_features']
    data_min = p.get("data_min", 1e-5)
    if self._both:
      n_feats = n_feats["magnitude"]
      if isinstance(data_min, dict):
        data_min = data_min["magnitude"]
      if not self._exp_mag:
        data_min = np.log(data_min)
    else:
      data_min = np.log(data_min)
    n_bins = self._n_fft // 2 + 1
    if n_feats < n_bins:
      spectrogram = np.pad(spectrogram, ((0, 0), (0, n_bins - spectrogram.shape[1])), "constant",
                           constant_values=data_min)
    mag_spec = spectrogram * 1.0 / p.get('mag_power', 2)
    if not self._both and not self._exp_mag:
      mag_spec = np.exp(mag_spec)
    return mag_spec

  def feature_sizes(self):
    naf = self.params['num_audio_features']
    if self._both:
      return naf['mel'], naf['magnitude']
    return (naf, 0) if self.params['output_type'] == 'mel' else (0, naf)

  def iterate_batches(self, device, seed=0, drop_remainder=None, num_batches=2):
    """eval / infer passes (run.py). The csv + wav reader of the reference's TTS data layer
    (data/text2speech/text2speech.py:150-420) is outside SURVEY 8f's file-reading row (ASR only): the
    pass runs over `num_batches` synthetic batches of the configured shapes."""
    for i in range(num_batches):
      yield self.synthetic_batch(device, seed + i)

  def synthetic_batch(self, device, seed, fixed_text=None, fixed_frames=None):
    p = self.params
    B = p['batch_size']
    rng = np.random.RandomState(seed)
    pad_to = p.get('pad_to', 8)
    V = p['src_vocab_size']
    sl = (np.full(B, fixed_text) if fixed_text else rng.randint(20, 201, size=B)).astype(np.int32)
    S = int(-(-sl.max() // pad_to) * pad_to)
    text = np.zeros((B, S), np.int32)
    for b in range(B):
      text[b, :sl[b] - 1] = rng.randint(3, V, size=sl[b] - 1)
      text[b, sl[b] - 1] = 2
    dmin, dmax = p.get('duration_min', 24), min(p.get('duration_max', 1024), 1024)
    raw = (np.full(B, fixed_frames) if fixed_frames else rng.randint(dmin, dmax + 1, size=B)).astype(np.int64)
    # pad_EOS: at least one EOS frame, total a multiple of pad_to (:494-536)
    num_pad = pad_to - ((raw + 1) % pad_to) + 1
    tl = (raw + num_pad).astype(np.int32) if p.get('pad_EOS', True) else raw.astype(np.int32)
    T = int(tl.max())
    n_mel, n_mag = self.feature_sizes()
    dm = p.get('data_min', 1e-5)
    dm_mel = dm['mel'] if isinstance(dm, dict) else dm
    dm_mag = dm['magnitude'] if isinstance(dm, dict) else dm
    feats = []
    if n_mel:
      mel = np.maximum(rng.randn(B, T, n_mel).astype(np.float32) - 2.0, math.log(dm_mel))
      feats.append(mel)
    if n_mag:
      lm = np.maximum(rng.randn(B, T, n_mag).astype(np.float32) - 3.0, math.log(dm_mag))
      feats.append(np.exp(lm) if self._exp_mag else lm)
    spec = np.concatenate(feats, -1)
    stop = np.zeros((B, T), np.float32)
    for b in range(B):
      if p.get('pad_EOS', True):
        spec[b, raw[b]:, :n_mel] = math.log(dm_mel)
        if n_mag:
          spec[b, raw[b]:, n_mel:] = dm_mag if self._exp_mag else math.log(dm_mag)
        stop[b, raw[b]:] = 1.0
      spec[b, tl[b]:] = 0.0
    t = lambda a: torch.from_numpy(a).to(device)
    src = [t(text), t(sl)]
    if p.get('style_input', None) == 'wav':
      src += [t(np.ascontiguousarray(spec[:, :, :n_mel])), t(tl)]
    return {'source_tensors': src, 'target_tensors': [t(spec), t(stop), t(tl)],
            'num_frames': int(tl.sum())}
