"""GPU tests of zoneout on the Tacotron 2 LSTMs against the float64 oracle of tests/_zoneout_cases.py: the
attention decoder's loop with sampled masks (forward + backward, every cell kernel: ad_cell_fwd, ti_lstm,
ad_cell_bwd, ad_cell_bwd_split) and with the expectation blend (stepped as the free-running fallback does), the
fused free-running decode, the encoder's LSTMCell layer (os2s_rnn_layer_{fwd,bwd}_zoneout) and one training
pass of a scaled-down Tacotron 2. Bounds are those of tests/_attn_decoder_cases.py compare() and of
tests/_rnn_cases.py for cell 2; every figure judged is printed.

Measured on the MI355X, the worst figure of each test next to its bound:
  decoder, mode 1   forward max err y 2.4e-2, ctx 7.7e-3 (3e-2 + 3e-2 |R|), align 1.6e-3 (5e-3 + 3e-2 |R|); gradients:
                    smallest cosine 0.9998 (> 0.99), largest rel 1.9e-2 (< 0.1), largest element error 3.9 % of
                    max|ref| (<= 10 %); kept c against the oracle's c_new 2.1e-2 (3e-2 + 3e-2 |R|); second backward,
                    state copies and mode 0 with p set: bit-identical
  decoder, mode 2   forward max err y 2.0e-2, ctx 7.6e-3, align 1.4e-3 (same bounds)
  fused decode      fused against step-wise: mel 3.1e-3, alignments 1.4e-4 (2e-2), post-net 3.8e-3 (5e-2); zoneout
                    moves the mel by 4.7e-2 (> 2e-2)
  encoder layer     largest err / bound: y 0.17, gates 0.16, c_seq 4.3e-3, h_seq 0.18, dgx 0 (bit-identical to R_b);
                    dWh against dg^T shift(h_seq) 2.6e-8 (bound 5.3e-4), against the shifted outputs 0.31
  train pass        loss 17.5027 with zoneout, 16.5306 without; two passes with the same seeds: the same bits"""
import pytest
import torch

import _zoneout_cases as Z

pytestmark = pytest.mark.gpu


def _report(fails):
  assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------ 5. decoder, mode 1
@pytest.mark.parametrize("name", sorted(Z.DEC_CASES))
def test_decoder_zoneout_sampled(cuda, name):
  case, p, _, _, option = Z.DEC_CASES[name]
  B, T, S, L, H = case[:5]
  fails = Z.masks_match_the_library((B, T, H), p, Z.SEEDS_H[:L] + Z.SEEDS_C[:L], cuda)
  fails += Z.dec_conditions(name)
  with Z.option_cleared(option):
    got = Z.run_dec(name, cuda, Z.SAMPLE)
    off_p = Z.run_dec(name, cuda, Z.OFF, p=p, second_backward=False)       # mode 0: p must not matter
    off_0 = Z.run_dec(name, cuda, Z.OFF, p=0.0, second_backward=False)
  R = Z.dec_reference(name, Z.SAMPLE)
  with Z.registered():
    fails += Z.adc.compare(name, got, R)
  fails += Z.state_copy_fails(name, got, R, Z.dec_masks(name))
  for k in sorted(off_0):
    pairs = zip(off_p[k], off_0[k]) if isinstance(off_0[k], list) else [(off_p[k], off_0[k])]
    for a, b in pairs:
      if a is not None and not Z.adc.same_bits(a, b):
        fails.append("%s: mode 0 with p = %g changes %s" % (name, p, k))
  if T > 1 and Z.adc.same_bits(got["y"], off_0["y"]):
    fails.append("%s: mode 1 left y as without zoneout" % name)
  _report(fails)


# ------------------------------------------------------------------------------------------ 6. decoder, mode 2
@pytest.mark.parametrize("name", Z.BLEND_CASES)
def test_decoder_zoneout_blend_stepwise(cuda, name):
  got = Z.run_dec(name, cuda, Z.BLEND, backward=False, stepwise=True)
  R = Z.dec_reference(name, Z.BLEND)
  fails = Z.forward_fails(name, got, R)
  whole = Z.run_dec(name, cuda, Z.BLEND, backward=False)
  for k in ("y", "ctx", "align"):
    if not Z.adc.same_bits(got[k], whole[k]):
      fails.append("%s: %s differs between one call per step and one call for all steps" % (name, k))
  _report(fails)


def test_decoder_backward_refuses_the_blend(cuda):
  from openseq2seq_amd import _lib
  with pytest.raises(_lib.Os2sError, match=r"os2s_attn_decoder_bwd failed: .*\(code -3\)$"):
    Z.run_dec("zo_t1", cuda, Z.BLEND, second_backward=False)


# ------------------------------------------------------------------------------------------ 7. fused decode
POST = [{"kernel_size": [5], "stride": [1], "num_channels": 64, "padding": "SAME", "activation_fn": "tanh"},
        {"kernel_size": [5], "stride": [1], "num_channels": -1, "padding": "SAME", "activation_fn": None}]


def _rel(a, b):
  a, b = a.float().cpu(), b.float().cpu()
  return float((a - b).norm() / (b.norm() + 1e-20))


def _build_decoder(cuda, zoneout, seed=5):
  """The scaled-down decoder of test_tacotron_infer_gpu.py::test_fused_decode_matches_stepwise_path with
  dropout_prob = 0 and the given zoneout_prob (same seed: same weights whatever the zoneout)."""
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  from openseq2seq_amd.decoders import Tacotron2Decoder
  H, M, P, NM, NG = 64, 128, 64, 16, 24
  torch.manual_seed(seed)
  store = FlatParams(cuda)
  dec = Tacotron2Decoder({"attention_layer_size": 128, "attention_type": "location", "attention_bias": True,
                          "decoder_cell_units": H, "decoder_cell_type": "LSTMCell", "decoder_layers": 2,
                          "dropout_prob": 0., "zoneout_prob": zoneout, "enable_prenet": True, "prenet_layers": 2,
                          "prenet_units": P, "enable_postnet": True, "postnet_keep_dropout_prob": 0.5,
                          "postnet_conv_layers": POST, "mask_decoder_sequence": False, "dtype": "mixed"}, None,
                         mode="eval")
  dec.build(store, memory_dim=M, num_audio_features={"mel": NM, "magnitude": NG}, exp_mag=False)
  store.finalize()
  g = torch.Generator().manual_seed(seed + 1)
  for p in store.params:
    if p.kind == "vector" and p.numel > 1 and "gamma" not in p.name:
      p.master.add_((torch.randn(p.shape, generator=g) * 0.1).to(cuda))
  # glorot-sized cell kernels keep the gates near their centres, where blending a tenth of the old state into
  # the new one moves the frames by less than the bound of the comparison (measured 1.7e-2 against 2e-2): three
  # times the kernels, so that a decode that ignored zoneout_prob could not pass
  with torch.no_grad():
    for w in [dec.cell.w_in] + dec.cell.wcat:
      w.master.mul_(3.0)
  store.refresh_compute_copies()
  return dec


def _decode(dec, mem, lens, cuda, steps):
  from openseq2seq_amd.parts.tape import Act
  enc = {"outputs": mem.to(cuda), "outputs_act": Act(mem.to(cuda), None, requires_grad=False), "src_length": lens.to(cuda)}
  out = dec.decode({"encoder_output": enc, "max_decoder_steps": steps})
  torch.cuda.synchronize()
  return out


def test_fused_decode_with_zoneout_matches_stepwise_path(cuda, monkeypatch):
  from openseq2seq_amd.decoders import tacotron2_decoder as t2d
  monkeypatch.setattr(t2d, "PRENET_KEEP", 1.0)
  B, S, M = 5, 18, 128
  lens = torch.tensor([18, 11, 15, 9, 18], dtype=torch.int32)
  g = torch.Generator().manual_seed(13)
  mem = torch.randn(B, S, M, generator=g) * 0.5
  mem = (mem * (torch.arange(S)[None, :] < lens[:, None]).float()[:, :, None]).to(torch.bfloat16)
  dec = _build_decoder(cuda, 0.1)
  a = _decode(dec, mem, lens, cuda, 16)
  monkeypatch.setenv("OS2S_TACOTRON_FUSED_DECODE", "0")
  b = _decode(dec, mem, lens, cuda, 16)
  monkeypatch.delenv("OS2S_TACOTRON_FUSED_DECODE")
  assert a["fused"] and not b["fused"]
  n = 10
  figs = (_rel(a["outputs"][0][:, :n], b["outputs"][0][:, :n]), _rel(a["outputs"][2][:, :n], b["outputs"][2][:, :n]),
          _rel(a["outputs"][1][:, :n], b["outputs"][1][:, :n]))
  plain = _decode(_build_decoder(cuda, 0.0), mem, lens, cuda, 16)
  assert plain["fused"]
  moved = _rel(a["outputs"][0][:, :n], plain["outputs"][0][:, :n])
  print("fused vs step-wise with zoneout: mel %.3e align %.3e post %.3e; zoneout moves the mel by %.3e" % (figs + (moved,)))
  assert figs[0] <= 2e-2 and figs[1] <= 2e-2 and figs[2] <= 5e-2, figs
  assert moved > 2e-2, moved


# ------------------------------------------------------------------------------------------ 8. encoder layer
def _rnn_zo(name, zmode):
  return [dict(mode=zmode, p=Z.RNN_P[zmode], **(m if zmode == Z.SAMPLE else {})) for m in Z.rnn_masks(name)]


@pytest.mark.parametrize("name", sorted(Z.RNN_CASES))
def test_encoder_layer_zoneout_sampled(cuda, name):
  B, T, H, _ = Z.RNN_CASES[name]
  d = Z.rnn_inputs(name)
  fails = Z.masks_match_the_library((B, T, H), Z.RNN_P[Z.SAMPLE], Z.RNN_SEEDS_H + Z.RNN_SEEDS_C, cuda)
  live = Z.rnn_live(name)
  for i, m in enumerate(Z.rnn_masks(name)):
    fails += Z.mask_conditions([m["mh"], m["mc"]], live, Z.RNN_P[Z.SAMPLE], "%s dir %d" % (name, i))
  got = Z.run_rnn(name, cuda, Z.SAMPLE)
  Rb = Z.rnn_forward_ref(name, Z.SAMPLE, True)
  for x, g, r, zo in zip(d["dirs"], got, Rb, _rnn_zo(name, Z.SAMPLE)):      # teacher-forced on the saved tensors
    r["dgx"] = Z.lstm_tf_zo_bwd(g["gates"], g["c_seq"], x["dy"], x["wh"], d["lens"], x["reverse"], zo, rounded=True)
  nq = Z.rc.noise_floor()[Z.rc.LSTM_TF]
  fails += Z.rnn_compare(name, got, Rb, nq, ("y", "gates", "c_seq", "h_seq", "dgx"))
  fails += Z.rnn_state_copy_fails(name, got, Z.rnn_masks(name))
  again = Z.run_rnn(name, cuda, Z.SAMPLE)
  for i, (a, b) in enumerate(zip(got, again)):
    for q in ("y", "h_seq", "dgx"):
      if not Z.adc.same_bits(a[q], b[q]):
        fails.append("%s dir %d: %s differs between two runs" % (name, i, q))
  _report(fails)


@pytest.mark.parametrize("name", sorted(Z.RNN_CASES))
def test_encoder_layer_zoneout_blend(cuda, name):
  got = Z.run_rnn(name, cuda, Z.BLEND, backward=False)
  Rb = Z.rnn_forward_ref(name, Z.BLEND, True)
  nq = Z.rc.noise_floor()[Z.rc.LSTM_TF]
  _report(Z.rnn_compare(name, got, Rb, nq, ("y", "gates", "c_seq", "h_seq")))


def test_encoder_layer_zoneout_entry_points_refuse_other_cells(cuda):
  from openseq2seq_amd import _lib, capi
  B, T, H = 2, 2, 8
  zo = dict(prob=0.5, mode=Z.SAMPLE, seeds_h=(1, 2), seeds_c=(3, 4))
  for cell, G in ((capi.CELL_GRU_CUDNN, 3), (capi.CELL_LSTM_CUDNN, 4)):
    gx = torch.zeros(B, T, G * H, dtype=torch.bfloat16, device=cuda)
    wh = torch.zeros(G * H, H, dtype=torch.bfloat16, device=cuda)
    with pytest.raises(_lib.Os2sError, match=r"os2s_rnn_layer_fwd_zoneout failed: .*\(code -3\)$"):
      capi.rnn_layer_fwd_multi(cell, [dict(gx=gx, wh=wh, bh=None, y=None, reverse=False)], None, H, zoneout=zo)


def test_recurrent_weight_gradient_comes_from_the_state_sequence(cuda, monkeypatch):
  """RNNDirection.weight_backward under zoneout: dWh = dg^T . (h_seq shifted by one step in processing order), in
  float64 from the launch's own dg and h_seq. fp32 accumulation over B T = 30 rows of bf16 products is good to
  a few 2^-24 of the sum of the terms' magnitudes: held to 1e-3 of max|ref|; the product with the shifted
  OUTPUTS y, which is what the parent forms, must miss that bound by more than ten times."""
  from openseq2seq_amd import capi
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  from openseq2seq_amd.parts.rnns.rnn_layers import RNNDirection, rnn_directions_forward
  from openseq2seq_amd.parts.tape import Act, Tape
  B, T, In, H = 5, 6, 16, 64
  torch.manual_seed(3)
  store = FlatParams(cuda)
  dirs = [RNNDirection(store, "zo/%s" % tag, "lstm_tf", [In], H, reverse=rev) for tag, rev in (("fw", False), ("bw", True))]
  store.finalize()
  g = torch.Generator().manual_seed(4)
  x = Act((torch.randn(B, T, In, generator=g)).to(torch.bfloat16).to(cuda), None)
  lens = torch.tensor([6, 1, 4, 6, 2], dtype=torch.int32)
  dys = [torch.randn(B, T, H, generator=g).to(torch.bfloat16).to(cuda) for _ in dirs]
  seen = {}
  fwd, bwd = capi.rnn_layer_fwd_multi, capi.rnn_layer_bwd_multi
  monkeypatch.setattr(capi, "rnn_layer_fwd_multi", lambda *a, **k: seen.setdefault("fwd", fwd(*a, **k)))
  monkeypatch.setattr(capi, "rnn_layer_bwd_multi", lambda *a, **k: seen.setdefault("bwd", bwd(*a, **k)))
  zo = dict(prob=0.5, mode=Z.SAMPLE, seeds_h=Z.RNN_SEEDS_H, seeds_c=Z.RNN_SEEDS_C)
  tape = Tape()
  store.zero_grads()
  outs = rnn_directions_forward(dirs, [x], lens.to(cuda), tape, zoneout=zo)
  for o, dy in zip(outs, dys):
    o.grad = dy
  tape.backward()
  torch.cuda.synchronize()
  for i, d in enumerate(dirs):
    y, h_seq = seen["fwd"][i][0].double().cpu(), seen["fwd"][i][3].double().cpu()
    dg = seen["bwd"][i][1].double().cpu()
    z = torch.zeros(B, 1, H, dtype=torch.float64)
    shift = (lambda t: torch.cat([t[:, 1:], z], 1)) if d.reverse else (lambda t: torch.cat([z, t[:, :-1]], 1))
    want = torch.einsum("btg,bth->gh", dg, shift(h_seq))
    parent = torch.einsum("btg,bth->gh", dg, shift(y))
    got = d.wh.grad.view(4 * H, H).double().cpu()
    bound = 1e-3 * float(want.abs().max())
    err, other = float((got - want).abs().max()), float((got - parent).abs().max())
    print("dir %d dWh: max err %.3e (bound %.3e); against the shifted outputs %.3e" % (i, err, bound, other))
    assert err <= bound and other > 10.0 * bound, (i, err, other, bound)


# ------------------------------------------------------------------------------------------ 9. end to end
def _train_pass(cuda, zoneout, seed):
  """Forward, loss and backward of the scaled-down Tacotron 2 of test_tacotron_e2e_gpu.py (encoder on the
  LSTMCell kernels): loss, outputs and the gradients of the zoned cells' recurrent weights."""
  from test_tacotron_e2e_gpu import CONVS, POST as POST3, SMALL as D
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  from openseq2seq_amd.encoders import Tacotron2Encoder
  from openseq2seq_amd.decoders import Tacotron2Decoder
  from openseq2seq_amd.losses import Text2SpeechLoss
  from openseq2seq_amd.parts.tape import Tape
  from openseq2seq_amd.parts.dense import SeedSeq
  torch.manual_seed(0)
  V, E, Henc, H, NM, NG = D["V"], D["E"], D["Henc"], D["H"], D["NM"], D["NG"]
  store = FlatParams(cuda)
  enc = Tacotron2Encoder({"cnn_dropout_prob": 0.0, "rnn_dropout_prob": 0.0, "src_emb_size": E, "conv_layers": CONVS,
                          "activation_fn": "relu", "num_rnn_layers": 1, "rnn_cell_dim": Henc, "use_cudnn_rnn": False,
                          "rnn_type": "LSTMCell", "rnn_unidirectional": False, "zoneout_prob": zoneout,
                          "dtype": "mixed"}, None, mode="train")
  enc.build(store, src_vocab_size=V, num_style_features=NM)
  dec = Tacotron2Decoder({"attention_layer_size": 128, "attention_type": "location", "attention_bias": True,
                          "decoder_cell_units": H, "decoder_cell_type": "LSTMCell", "decoder_layers": 2,
                          "dropout_prob": 0.0, "zoneout_prob": zoneout, "enable_prenet": True, "prenet_layers": 2,
                          "prenet_units": D["pre"], "enable_postnet": True, "postnet_keep_dropout_prob": 1.0,
                          "postnet_conv_layers": POST3, "dtype": "mixed"}, None, mode="train")
  dec.build(store, memory_dim=enc.output_dim, num_audio_features={"mel": NM, "magnitude": NG}, exp_mag=True)
  lossf = Text2SpeechLoss({"use_mask": True, "dtype": "mixed"}, None)
  store.finalize()
  g = torch.Generator().manual_seed(2)
  for p in store.params:
    if p.kind == "vector" and p.numel > 1 and "gamma" not in p.name:
      p.master.add_((torch.randn(p.shape, generator=g) * 0.1).to(cuda))
  store.refresh_compute_copies()
  B, S, T = D["B"], D["S"], D["T"]
  text = torch.randint(3, V, (B, S), generator=g).to(torch.int32)
  text_len = torch.tensor(D["text_len"], dtype=torch.int32)
  spec_len = torch.tensor(D["spec_len"], dtype=torch.int32)
  spec = torch.cat([torch.randn(B, T, NM, generator=g) - 1.0, torch.exp(torch.randn(B, T, NG, generator=g) - 2.0)], -1)
  spec = spec.to(torch.bfloat16).float()
  stop = (torch.arange(T)[None, :] >= (spec_len[:, None] - 2)).float()
  tape = Tape()
  store.zero_grads()
  e = enc.encode({"source_tensors": [text.to(cuda), text_len.to(cuda)], "tape": tape, "seeds": SeedSeq(seed)})
  tgt = [spec.to(cuda), stop.to(cuda), spec_len.to(cuda)]
  d = dec.decode({"encoder_output": e, "target_tensors": tgt, "tape": tape})
  L = lossf.compute_loss({"decoder_output": d, "target_tensors": tgt})
  tape.backward()
  torch.cuda.synchronize()
  out = {"loss": L.float().cpu().clone(), "mel": d["outputs"][0].cpu().clone(), "align": d["outputs"][2].cpu().clone(),
         "encoder": e["outputs"].cpu().clone()}
  for w in dec.cell.wcat + [dd.wh for dd in enc.rnn[0]]:
    out["grad " + w.name] = w.grad.cpu().clone()
  return out


def test_tacotron2_train_pass_with_zoneout(cuda):
  a = _train_pass(cuda, 0.1, seed=5)
  b = _train_pass(cuda, 0.1, seed=5)
  plain = _train_pass(cuda, 0.0, seed=5)
  assert bool(torch.isfinite(a["loss"]).all()) and all(bool(torch.isfinite(v.float()).all()) for v in a.values())
  differ = [k for k in a if not Z.adc.same_bits(a[k], b[k])]
  print("loss with zoneout %.6f, without %.6f" % (float(a["loss"].flatten()[0]), float(plain["loss"].flatten()[0])))
  assert not differ, differ
  assert not Z.adc.same_bits(a["loss"], plain["loss"])
  assert not Z.adc.same_bits(a["encoder"], plain["encoder"]) and not Z.adc.same_bits(a["mel"], plain["mel"])
