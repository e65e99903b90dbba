"""CPU checks of tests/_tacotron_step_cases.py, the stage-wise float64 oracle of the free-running Tacotron 2
decode step (no GPU):

  * the conditions on the inputs hold for every case (check_inputs: dot allowances at most 2^-10 rms(R), no
    saturated softmax, gate pre-activations with an rms in [0.3, 3], stop logits of the mask-sequence cases
    away from zero, src_len with 1 and S);
  * the stage oracle, chained over T steps from zero state, agrees with oracle.tacotron.decoder_infer (the
    oracle pinned to the reference's own code) to 1e-9 in float64;
  * compare() is not vacuous: it passes the oracle's own outputs rounded as the device stores them, and
    fails for each kernel mistake of MUTATIONS built into such a result.

The pre-net masks are seeded stand-ins here (the library's need the device). The mutation "column" replaces
the last sample's input row by its neighbour's: column 16 by column 15 on b17 (the second MFMA column tile),
column 2 by column 1 on the three-sample cases."""
import pytest
import torch

import _tacotron_step_cases as C
from oracle import tacotron as otac

ALL = sorted(C.CASES)


def _quiet(*a):
  pass


@pytest.mark.parametrize("case", ALL)
def test_inputs_cpu(case):
  bad = C.check_inputs(case)
  assert not bad, "\n".join(bad)


def test_mask_sequence_cases_exercise_the_stop_token():
  a, b = C.chain("mask_seq_a"), C.chain("mask_seq_b")
  T = C.CASES["mask_seq_a"]["T"]
  assert 1 < a["n_run"] < T, a["n_run"]                    # a: ends early, rows of later steps are never written
  assert b["n_run"] == T and int(b["state"][1]) == 0       # b: a sample never finishes
  assert 0 < int(b["state"][2]) < C.CASES["mask_seq_b"]["B"]


@pytest.mark.parametrize("case", ["base", "b17"])
def test_stage_oracle_agrees_with_decoder_infer(case):
  B, S, H, M, P, nm, K, F, T = C.dims(case)
  W = C.oracle_weights(case)
  G = C.chain(case, exact=True)
  cell = dict(wcat=[W["w0x"][:, P:], W["wcat1"]], bias=[None, W["bias1"]], wq=W["wq"], wmem=W["wmem"], v=W["v"],
              b=W["b"], conv_w=W["conv_w"], conv_b=W["conv_b"], dense_w=W["dense_w"], w_in=W["w0x"][:, :P],
              b0=W["bias0"])
  Pm = {"prenet": [(W["wp1"], W["bp1"]), (W["wp2"], W["bp2"])], "cell": cell, "out_w": W["wout"], "out_b": W["bout"],
        "stop_w": W["wstop"][None, :], "stop_b": W["bstop"]}
  ref = otac.decoder_infer(Pm, W["values"], W["src_len"], max_steps=T, prenet_masks=C.prenet_masks(case, None),
                           mask_decoder_sequence=False, round_frames_bf16=True)
  assert ref["mel"].dtype == torch.float64
  for k in ("mel", "stop", "align"):
    err = float((G[k] - ref[k]).abs().max())
    assert err <= 1e-9, (k, err)
  assert ref["lengths"].tolist() == [T] * B


@pytest.mark.parametrize("case", ["base", "k2624", "b17", "mask_seq_a", "zoneout_blend", "k2112_e4m3"])
def test_compare_passes_the_oracle_rounded_as_the_device_stores(case):
  lines = []
  fails = C.compare(case, C.chain(case), log=lambda s: lines.append(s))
  assert not fails, "\n".join(fails)
  assert any("worst err/E" in s for s in lines)


@pytest.mark.parametrize("mut", C.MUTATIONS)
@pytest.mark.parametrize("case", ["base", "k2624"])
def test_compare_fails_for_a_kernel_mistake(case, mut):
  fails = C.compare(case, C.chain(case, mut=mut), log=_quiet)
  assert fails, "compare() passes a result with the mistake %r built in" % mut
  print("%s / %s: %d failures, first: %s" % (case, mut, len(fails), fails[0]))


def test_compare_fails_for_column_16_read_from_column_15():
  fails = C.compare("b17", C.chain("b17", mut="column"), log=_quiet)
  assert any("cell 0" in f for f in fails), fails


def test_forced_geometry_depths():
  """d of ti_lstm_kernel follows the geometry the launcher picks: by K, or the forced one."""
  assert C.lstm_geom(2048) == (8, 4) and C.lstm_geom(2112) == (9, 4) and C.lstm_geom(2304) == (9, 4)
  assert C.lstm_geom(2368) == (8, 5) and C.lstm_geom(2624) == (8, 5)
  assert C.d_lstm(2624, False) == 32 + 2 * 5 * 2 + 8 + 1
  assert C.d_lstm(2112, True, ("geom", 1602)) == 32 + 2 * 2 * 2 + 16 + 2
  assert C.lstm_geom(2112, ("geom", 805)) == (8, 5) and C.lstm_geom(2112, ("rows", 32)) == (8, 5)
