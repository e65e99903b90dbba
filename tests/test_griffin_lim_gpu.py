"""GPU tests of the Griffin-Lim vocoder (csrc/griffin_lim.hip, models/text2speech.py) against the float64
restatement of librosa's stft / istft in _griffin_lim_ref.py.

Bounds. The device computes in fp32 like librosa does (complex64), so its distance from the float64 run is
compared with that of the float32 emulation of the same algorithm ON THE SAME INPUT: <= 8 x the emulation's
error (the device sums its dot products in another order), with a floor of 1e-5 for the 50-iteration runs.
Magnitudes are the STFT magnitudes of a seeded harmonic-plus-noise signal; on such inputs the iteration is not
chaotic (the emulation stays within 2e-5 of float64 after 50 iterations), so whole-run parity is a fair test.
The kernels tile frames by 64: the ragged batches hold T = 4 (the minimum), 63, 64 and 65."""
import os
import struct

import numpy as np
import pytest
import torch

import _griffin_lim_ref as glr

pytestmark = pytest.mark.gpu

TILE = 64      # frames per tile of both kernels


def _case(n_fft, T, seed):
  _, mag, ph = glr.make_signal(n_fft, T, seed)
  return mag.astype(np.float32), ph.astype(np.float32)      # what the device is given, exactly


def _batch(cases, cuda, n_iters, n_fft, **kw):
  """cases: list of (mag [K, T], phase [K, T]) -> list of signals (NumPy), flags."""
  from openseq2seq_amd.models.text2speech import griffin_lim_batch
  K = n_fft // 2 + 1
  lens = [m.shape[1] for m, _ in cases]
  T = max(lens)
  mags = np.zeros((len(cases), T, K), np.float32)
  phs = np.zeros((len(cases), T, K), np.float32)
  for b, (m, p) in enumerate(cases):
    mags[b, :lens[b]], phs[b, :lens[b]] = m.T, p.T
  sig, flags = griffin_lim_batch(torch.from_numpy(mags).to(cuda), lens, n_iters, n_fft, phase=phs, **kw)
  sig, flags = sig.cpu().numpy(), flags.cpu().numpy()
  hop = n_fft // 4
  for b in range(len(cases)):
    assert not sig[b, hop * (lens[b] - 1):].any(), "samples past the utterance's end must be zero"
  return [sig[b, :hop * (lens[b] - 1)] for b in range(len(cases))], flags


@pytest.mark.parametrize("n_fft,T", [(64, 37), (800, 21), (1024, 9)])
@pytest.mark.parametrize("n_iters", [0, 1])
def test_primitives_match_fp64(cuda, n_fft, T, n_iters):
  """n_iters = 0 is the istft alone, n_iters = 1 adds one stft + projection + istft."""
  mag, ph = _case(n_fft, T, 3)
  ref = glr.griffin_lim(mag, ph, n_iters, n_fft)
  emu = glr.rel_l2(glr.griffin_lim_fp32(mag, ph, n_iters, n_fft), ref)
  (got,), flags = _batch([(mag, ph)], cuda, n_iters, n_fft)
  err = glr.rel_l2(got, ref)
  print("griffin_lim n_fft %d T %d n_iters %d: device vs fp64 %.3e, fp32 emulation vs fp64 %.3e" % (n_fft, T, n_iters, err, emu))
  assert flags[0] == 0 and got.dtype == np.float32
  assert err <= 8 * emu, (err, emu)


@pytest.mark.parametrize("n_fft,frames", [(64, (4, TILE - 1, TILE, TILE + 1)), (800, (21, 9)), (1024, (9,))])
def test_whole_run_ragged_batch(cuda, n_fft, frames):
  """50 iterations on a ragged batch: every utterance equals its own B = 1 run bit for bit (no leakage from
  padding or batch-mates), stays within the fp32 bound of the float64 run, and converges as far as it does."""
  cases = [_case(n_fft, T, 10 + i) for i, T in enumerate(frames)]
  got, flags = _batch(cases, cuda, 50, n_fft)
  assert not flags.any()
  for (mag, ph), g, T in zip(cases, got, frames):
    (alone,), _ = _batch([(mag, ph)], cuda, 50, n_fft)
    assert np.array_equal(alone, g), "T = %d differs from its B = 1 run" % T
    ref = glr.griffin_lim(mag, ph, 50, n_fft)
    emu = glr.rel_l2(glr.griffin_lim_fp32(mag, ph, 50, n_fft), ref)
    err = glr.rel_l2(g, ref)
    sc_dev, sc_ref = glr.spectral_convergence(g, mag, n_fft), glr.spectral_convergence(ref, mag, n_fft)
    print("griffin_lim n_fft %d T %d, 50 iterations: device vs fp64 %.3e, fp32 emulation vs fp64 %.3e, "
          "spectral convergence device %.6f reference %.6f" % (n_fft, T, err, emu, sc_dev, sc_ref))
    assert err <= max(8 * emu, 1e-5), (T, err, emu)
    assert sc_dev <= 1.01 * sc_ref, (T, sc_dev, sc_ref)


def test_zero_magnitude_block_is_finite_and_silent(cuda):
  """Where every magnitude is zero |X| == 0 takes the 1 + 0j branch: the signal there is finite and zero."""
  n_fft, T = 64, 40
  mag, ph = _case(n_fft, T, 5)
  mag[:, 12:30] = 0.0
  (got,), flags = _batch([(mag, ph)], cuda, 3, n_fft)
  hop = n_fft // 4
  assert flags[0] == 0 and np.isfinite(got).all()
  # frames 12 .. 29 are silent; samples covered only by them: padded blocks 15 .. 29 = samples hop * 13 .. hop * 28
  assert not got[hop * 13:hop * 28].any()
  assert np.abs(got[:hop * 8]).max() > 1e-3
  (allzero,), flags = _batch([(np.zeros_like(mag), ph)], cuda, 2, n_fft)
  assert flags[0] == 0 and not allzero.any()


def test_inf_magnitude_flags_its_utterance_only(cuda):
  from openseq2seq_amd.models.text2speech import griffin_lim
  n_fft = 64
  cases = [_case(n_fft, T, 20 + i) for i, T in enumerate((17, 9, 30))]
  clean, _ = _batch(cases, cuda, 4, n_fft)
  bad = [(m.copy(), p) for m, p in cases]
  bad[1][0][7, 3] = np.inf
  got, flags = _batch(bad, cuda, 4, n_fft)
  assert flags.tolist() == [0, 1, 0]
  assert np.array_equal(got[0], clean[0]) and np.array_equal(got[2], clean[2])
  out = griffin_lim(bad[1][0], n_iters=2, n_fft=n_fft, phase=bad[1][1])
  assert out.shape == (1,) and out[0] == 0
  ok = griffin_lim(cases[1][0], n_iters=4, n_fft=n_fft, phase=cases[1][1])
  assert np.array_equal(ok, clean[1])


def test_two_runs_are_bit_identical(cuda):
  n_fft = 800
  cases = [_case(n_fft, T, 30 + i) for i, T in enumerate((13, 70))]
  a, _ = _batch(cases, cuda, 5, n_fft)
  b, _ = _batch(cases, cuda, 5, n_fft)
  assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_seeded_phase_and_clip_power(cuda):
  """phase=None draws np.random.rand (a seeded np.random reproduces); clip / power run on the device."""
  from openseq2seq_amd.models.text2speech import griffin_lim, griffin_lim_batch
  n_fft = 64
  mag, _ = _case(n_fft, 12, 40)
  np.random.seed(7)
  a = griffin_lim(mag, n_iters=2, n_fft=n_fft)
  np.random.seed(7)
  ph = np.random.rand(*mag.shape)
  assert np.array_equal(a, griffin_lim(mag, n_iters=2, n_fft=n_fft, phase=ph))
  big = (mag * 100.0 - 5.0).astype(np.float32)
  host = (np.clip(big, 0, 255).astype(np.float64) ** 1.5)
  ref = glr.griffin_lim(host, ph, 2, n_fft)
  sig, _ = griffin_lim_batch(torch.from_numpy(big.T[None].copy()).to(cuda), [12], 2, n_fft, power=1.5,
                             phase=ph.T[None], clip_max=255.0)
  assert glr.rel_l2(sig[0].cpu().numpy(), ref) <= 1e-5


def _read_wav(path):
  raw = open(path, "rb").read()
  assert raw[:4] == b"RIFF" and raw[8:12] == b"WAVE"
  pos, out = 12, {}
  while pos < len(raw):
    tag, size = raw[pos:pos + 4], struct.unpack("<I", raw[pos + 4:pos + 8])[0]
    out[tag] = raw[pos + 8:pos + 8 + size]
    pos += 8 + size
  fmt = struct.unpack("<HHIIHH", out[b"fmt "][:16])
  return fmt, np.frombuffer(out[b"data"], "<f4")


def test_infer_writes_wav_files(cuda, tmp_path):
  """run.py --mode=infer on a toy Tacotron 2 "both" model: two synthetic batches through infer_batch, then
  finalize_inference writes sample_step0_{n}_infer.wav and ..._infer_mag.wav of hop * (length - 2) samples for
  every sample with enough frames."""
  from openseq2seq_amd.configs.tacotron import tacotron_gst_config
  model_cls, params = tacotron_gst_config(batch_size_per_gpu=3, style=False)
  conv = lambda c, act: {"kernel_size": [5], "stride": [1], "num_channels": c, "padding": "SAME", "activation_fn": act}
  enc_conv = {"kernel_size": [5], "stride": [1], "num_channels": 64, "padding": "SAME"}
  params["encoder_params"].update({"src_emb_size": 64, "conv_layers": [enc_conv] * 2, "rnn_cell_dim": 32})
  # random weights make the stop token meaningless: run every sample for the given number of steps
  params["decoder_params"].update({"decoder_cell_units": 64, "prenet_units": 64, "mask_decoder_sequence": False,
                                   "postnet_conv_layers": [conv(64, "tanh")] * 2 + [conv(-1, None)]})
  n_fft = 64
  params["data_layer_params"].update({"dataset": "LJ", "n_fft": n_fft, "num_audio_features": {"mel": 16, "magnitude": 33}})
  params["logdir"] = str(tmp_path)
  model = model_cls(params, mode="infer", hvd=None, device=cuda)
  model.compile()
  dl = model.get_data_layer()
  assert dl.n_fft == n_fft and dl.sampling_rate == 22050
  results = [model.infer_batch(dl.synthetic_batch(cuda, seed=s, fixed_text=10), max_decoder_steps=steps)
             for s, steps in ((1, 9), (2, 14))]
  model.finalize_inference(results, None)
  expected = 0
  for i, res in enumerate(results):
    for j, length in enumerate(res["outputs"][4].cpu().tolist()):
      for mode in ("infer", "infer_mag"):
        path = os.path.join(str(tmp_path), "sample_step0_%d_%s.wav" % (i * 3 + j, mode))
        if length - 1 >= 4:
          fmt, data = _read_wav(path)
          assert fmt[0] == 3 and fmt[1] == 1 and fmt[2] == 22050 and fmt[5] == 32
          assert len(data) == (n_fft // 4) * (length - 2) and np.isfinite(data).all()
          expected += 1
        else:
          assert not os.path.exists(path)
  assert expected >= 2, "the case must write audio"
