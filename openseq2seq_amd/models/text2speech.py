"""Text2Speech / Text2SpeechTacotron — open_seq2seq/models/text2speech.py:111-413,
text2speech_tacotron.py. The model shell (feature sizes flow from the data layer to the decoder and the loss),
and the audio end of the infer mode: `griffin_lim` / `save_audio` (:111-198) and `finalize_inference` (:339-413)
turn the predicted spectrograms into wav files in logdir. The Griffin-Lim iterations run on the GPU
(csrc/griffin_lim.hip: a whole ragged batch per call, exact fp32); the plots and the image / audio summaries built from
them are not provided (the scalar and histogram summaries of training are: utils/summary.py). The reference defines no objects-per-step for TTS; benchmarks here count target mel frames."""
from __future__ import absolute_import, division, print_function

import struct

import numpy as np
import torch

from .. import capi
from .encoder_decoder import EncoderDecoderModel
from ..parts.dense import SeedSeq

GL_MIN_FRAMES = 4        # reflect padding needs hop * (T - 1) > n_fft / 2 (np.pad fails below that in the reference too)
_gl_tables = {}


def _check_n_fft(n_fft):
  if n_fft % 8 != 0 or not 64 <= n_fft <= 2048:
    raise ValueError("griffin_lim: n_fft must be a multiple of 8 with 64 <= n_fft <= 2048, got %r" % (n_fft,))


def griffin_lim_tables(n_fft, device):
  """The constant operands of os2s_griffin_lim (layouts: include/os2s.h), computed in fp64 and rounded once:
  windowed analysis basis, Hermitian-weighted windowed synthesis basis, 1 / window sum-of-squares for the first,
  an interior and the last hop block istft keeps. Cached per (device, n_fft)."""
  key = (str(device), n_fft)
  if key not in _gl_tables:
    K, hop = n_fft // 2 + 1, n_fft // 4
    Kp, hopP = capi.griffin_lim_pads(n_fft)
    n = np.arange(n_fft)
    win = 0.5 - 0.5 * np.cos(2 * np.pi * n / n_fft)            # periodic Hann: librosa's default window
    ang = 2 * np.pi * ((n[:, None] * np.arange(K)[None, :]) % n_fft) / n_fft       # [n_fft, K]
    A = np.zeros((n_fft, 2 * Kp))
    A[:, :K] = np.cos(ang) * win[:, None]
    A[:, Kp:Kp + K] = -np.sin(ang) * win[:, None]
    w = np.full(K, 2.0)
    w[0] = w[-1] = 1.0
    S = np.zeros((2 * Kp, 4, hopP))
    S[:K, :, :hop] = ((w[:, None] / n_fft) * np.cos(ang).T * win[None, :]).reshape(K, 4, hop)
    S[Kp:Kp + K, :, :hop] = (-(w[:, None] / n_fft) * np.sin(ang).T * win[None, :]).reshape(K, 4, hop)
    w2 = (win ** 2).reshape(4, hop)
    wss = np.ones((3, hopP))
    wss[0, :hop] = w2[0] + w2[1] + w2[2]      # padded block 2: frames 2, 1, 0
    wss[1, :hop] = w2.sum(0)
    wss[2, :hop] = w2[1] + w2[2] + w2[3]      # padded block T: frames T-1, T-2, T-3
    # librosa leaves samples whose window sum is below tiny() undivided
    inv = np.where(wss > np.finfo(np.float32).tiny, 1.0 / np.maximum(wss, 1e-300), 1.0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
    _gl_tables[key] = (t(A), t(S), t(inv))
  return _gl_tables[key]


def griffin_lim_batch(mags, lengths, n_iters, n_fft, power=1.0, phase=None, clip_max=None):
  """Griffin-Lim on a ragged batch in one call: mags fp32 [B, T, n_fft/2 + 1] (device), lengths [B] frames per
  utterance. M = clip(mags, 0, clip_max) ** power (no clipping when clip_max is None); `phase` [B, T, K] in
  [0, 1) is the initial phase in turns, drawn with np.random.rand when None (a seeded np.random reproduces).
  Returns (signal fp32 [B, hop * (T - 1)], flags int32 [B]) on the device: utterance b fills the first
  hop * (lengths[b] - 1) samples; flags[b] = 1 where the audio was not finite."""
  _check_n_fft(n_fft)
  if mags.dim() != 3 or mags.shape[2] != n_fft // 2 + 1:
    raise ValueError("griffin_lim: magnitudes must be [B, T, n_fft/2 + 1 = %d], got %s"
                     % (n_fft // 2 + 1, tuple(mags.shape)))
  B, T, _ = mags.shape
  lens = [int(v) for v in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
  if len(lens) != B or min(lens) < GL_MIN_FRAMES or max(lens) > T:
    raise ValueError("griffin_lim: every utterance needs %d <= frames <= %d, got %s" % (GL_MIN_FRAMES, T, lens))
  dev = mags.device
  if phase is None:
    phase = np.random.rand(B, T, mags.shape[2])
  if not torch.is_tensor(phase):
    phase = torch.from_numpy(np.ascontiguousarray(phase, dtype=np.float32))
  phase = phase.to(device=dev, dtype=torch.float32).contiguous()
  A, S, inv = griffin_lim_tables(n_fft, dev)
  lens_dev = torch.tensor(lens, dtype=torch.int32, device=dev)
  return capi.griffin_lim(mags.to(torch.float32).contiguous(), lens_dev, phase, A, S, inv, n_fft=n_fft,
                          n_iters=n_iters, power=power, clip_max=0.0 if clip_max is None else clip_max)


def griffin_lim(magnitudes, n_iters=50, n_fft=1024, phase=None):
  """text2speech.py:182-198. magnitudes [n_fft/2 + 1, T] NumPy; returns the signal (fp32 NumPy, hop * (T - 1)
  samples), or np.array([0.]) when the audio is not finite. `phase` [K, T] in [0, 1) replaces the
  np.random.rand draw."""
  magnitudes = np.asarray(magnitudes)
  if phase is None:
    phase = np.random.rand(*magnitudes.shape)
  if magnitudes.ndim != 2:
    raise ValueError("griffin_lim: magnitudes must be [n_fft/2 + 1, T], got %s" % (magnitudes.shape,))
  dev = torch.device("cuda", torch.cuda.current_device())
  m = torch.from_numpy(np.ascontiguousarray(magnitudes.T, dtype=np.float32))[None].to(dev)
  ph = np.ascontiguousarray(np.asarray(phase).T, dtype=np.float32)[None]
  signal, flags = griffin_lim_batch(m, [magnitudes.shape[1]], n_iters, n_fft, phase=ph)
  if int(flags[0].item()):
    print("WARNING: audio was not finite, skipping audio saving")
    return np.array([0.])
  return signal[0].cpu().numpy()


def write_wav(file_name, sampling_rate, signal):
  """What scipy.io.wavfile.write(file_name, rate, float32 array) produces: RIFF / WAVE with an 18-byte fmt chunk
  of format tag 3 (IEEE float), one channel, 32 bits, a fact chunk with the sample count, and the data chunk."""
  data = np.ascontiguousarray(signal, dtype="<f4").tobytes()
  n = len(data) // 4
  fmt = struct.pack("<HHIIHHH", 3, 1, int(sampling_rate), int(sampling_rate) * 4, 4, 32, 0)
  body = (b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"fact" + struct.pack("<II", 4, n)
          + b"data" + struct.pack("<I", len(data)) + data)
  with open(file_name, "wb") as f:
    f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def _emit_audio(signal, logdir, step, sampling_rate, mode, number, save_format, max_normalization):
  """The tail of save_audio (:154-179) on a finished signal."""
  if max_normalization:
    signal = signal / np.max(np.abs(signal))
  if save_format == "np.array":
    return signal
  if save_format == "disk":
    file_name = '{}/sample_step{}_{}_{}.wav'.format(logdir, step, number, mode)
    if logdir[0] != '/':
      file_name = "./" + file_name
    write_wav(file_name, sampling_rate, signal)
    return None
  print(("WARN: The save format passed to save_audio was not understood. No "
         "sound files will be saved for the current step. "
         "Received '{}'."
         "Expected one of 'np.array' or 'disk' ('tensorboard' needs TensorFlow)").format(save_format))
  return None


def save_audio(magnitudes, logdir, step, sampling_rate, n_fft=1024, mode="train", number=0, save_format="disk",
               power=1.5, gl_iters=50, verbose=True, max_normalization=False):
  """text2speech.py:111-179: magnitudes [time, n_fft/2 + 1] -> Griffin-Lim audio, returned ("np.array") or
  written to {logdir}/sample_step{step}_{number}_{mode}.wav ("disk")."""
  magnitudes = np.asarray(magnitudes)
  if np.min(magnitudes) < 0 or np.max(magnitudes) > 255:
    if verbose:
      print("WARNING: {} audio was clipped at step {}".format(mode.capitalize(), step))
    magnitudes = np.clip(magnitudes, a_min=0, a_max=255)
  signal = griffin_lim(magnitudes.T ** power, n_iters=gl_iters, n_fft=n_fft)
  return _emit_audio(signal, logdir, step, sampling_rate, mode, number, save_format, max_normalization)


class Text2Speech(EncoderDecoderModel):
  @staticmethod
  def get_required_params():
    return dict(EncoderDecoderModel.get_required_params(), **{})

  def _build_forward_pass_objects(self, store):
    self._data_layer = self._create_data_layer()
    self._encoder = self._create_encoder()
    self._decoder = self._create_decoder()
    if self.mode in ("train", "eval"):
      self._loss_computator = self._create_loss()
    self._encoder.build(store)
    self._decoder.build(store, memory_dim=self._encoder.output_dim)

  def _forward_backward(self, batch, tape):
    seeds = SeedSeq(self._seed * 7919 + self._step_count)
    enc = self._encoder.encode({'source_tensors': batch['source_tensors'], 'tape': tape,
                                'seeds': seeds})
    dec = self._decoder.decode({'encoder_output': enc, 'target_tensors': batch['target_tensors'],
                                'tape': tape})
    scale_dev = self._train_op.loss_scale_view if self._train_op is not None else None
    return self._loss_computator.compute_loss({
        'decoder_output': dec, 'target_tensors': batch['target_tensors'],
        'loss_scale_dev': scale_dev})

  def infer_batch(self, batch, max_decoder_steps=None):
    """infer (text2speech.py:205-317; finalize_inference turns the outputs into audio): free-running
    decode of one batch. max_decoder_steps overrides the reference's 10 x max(src_len) cap (benchmarks)."""
    enc = self._encoder.encode({'source_tensors': batch['source_tensors']})
    return self._decoder.decode({'encoder_output': enc, 'max_decoder_steps': max_decoder_steps})

  def finalize_inference(self, results_per_batch, output_file, power=1.5, gl_iters=50):
    """text2speech.py:339-413 without the plots: for every sample with length > 2 write
    {logdir}/sample_step0_{n}_infer.wav from the post-net mel frames [:length - 1] through
    get_magnitude_spec(is_mel=True), and for output_type "both" also ..._infer_mag.wav from the magnitude
    output. `results_per_batch` holds what infer_batch returned per batch; each batch's utterances go through
    Griffin-Lim in one call. Samples left with fewer than 4 frames cannot be reflect-padded and are skipped."""
    print("output_file is ignored for tts")
    print("results are logged to the logdir")
    dl = self.get_data_layer()
    logdir = self.params["logdir"]
    both = "both" in dl.params["output_type"]
    batch_size = None
    for i, res in enumerate(results_per_batch):
      outputs = res["outputs"] if isinstance(res, dict) else res[1]
      post = outputs[1].float().cpu().numpy()
      lengths = [int(v) for v in outputs[4].cpu().tolist()]
      mag_out = outputs[5].float().cpu().numpy() if both else None
      if batch_size is None:
        batch_size = post.shape[0]
      jobs = []                                   # (sample number, mode, magnitudes [frames, K])
      for j, length in enumerate(lengths):
        number = i * batch_size + j
        if length <= 2:
          continue
        if length - 1 < GL_MIN_FRAMES:
          print("WARNING: sample %d has %d frames, fewer than the %d Griffin-Lim needs: no audio saved"
                % (number, length - 1, GL_MIN_FRAMES))
          continue
        if both:
          jobs.append((number, "infer_mag", mag_out[j, :length - 1, :].astype(float)))
        jobs.append((number, "infer", dl.get_magnitude_spec(post[j, :length - 1, :], is_mel=True)))
      if not jobs:
        continue
      K = dl.n_fft // 2 + 1
      T = max(m.shape[0] for _, _, m in jobs)
      mags = np.zeros((len(jobs), T, K), np.float32)
      for n, (number, mode, m) in enumerate(jobs):
        if m.shape[1] != K:
          raise ValueError("finalize_inference: %d magnitude bins, n_fft %d needs %d" % (m.shape[1], dl.n_fft, K))
        if np.min(m) < 0 or np.max(m) > 255:
          print("WARNING: {} audio was clipped at step {}".format(mode.capitalize(), 0))
        mags[n, :m.shape[0]] = m
      signal, flags = griffin_lim_batch(torch.from_numpy(mags).to(self._device), [m.shape[0] for _, _, m in jobs],
                                        gl_iters, dl.n_fft, power=power, clip_max=255.0)
      signal, flags = signal.cpu().numpy(), flags.cpu().numpy()
      for n, (number, mode, m) in enumerate(jobs):
        if flags[n]:
          print("WARNING: audio was not finite, skipping audio saving")
          wav = np.array([0.], np.float32)
        else:
          wav = signal[n, :(dl.n_fft // 4) * (m.shape[0] - 1)]
        _emit_audio(wav, logdir, 0, dl.sampling_rate, mode, number, "disk",
                    dl.max_normalization and not flags[n])

  def evaluate_batch(self, batch):
    """Eval mode of the reference graph (utils/funcs.py:293-340 sums `eval_losses`): free-running decode,
    then Text2SpeechLoss with prediction and target padded to a common length
    (losses/text2speech_loss.py:80-131). Returns (loss, target frames)."""
    enc = self._encoder.encode({'source_tensors': batch['source_tensors']})
    dec = self._decoder.decode({'encoder_output': enc})
    loss = self._loss_computator.compute_loss({'decoder_output': dec, 'target_tensors': batch['target_tensors'],
                                               'want_grad': False})
    return float(loss.cpu()[0]), int(batch['target_tensors'][2].sum().item())

  def evaluate(self, device=None, max_batches=None):
    """One pass over the eval data layer (run.py --mode=eval / train_eval): mean eval loss per batch,
    'Validation loss' of utils/funcs.py:335-340."""
    dl = self.get_data_layer()
    losses, frames = [], 0
    for n, batch in enumerate(dl.iterate_batches(device or self._device, drop_remainder=False)):
      if max_batches is not None and n >= max_batches:
        break
      l, f = self.evaluate_batch(batch)
      losses.append(l)
      frames += f
    return {"eval_loss": sum(losses) / max(len(losses), 1), "batches": len(losses), "target_frames": frames}

  def _get_num_objects_per_step(self, batch):
    return batch['target_tensors'][2].sum()


class Text2SpeechTacotron(Text2Speech):
  pass
