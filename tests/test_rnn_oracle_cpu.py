"""The bound of tests/_rnn_cases.py can fail: compare() is fed, in place of a device result, the output of a
deliberately wrong float64 recurrence (rounded like R_b, so the mutation is the only difference) and must
reject every one of them on h8, b33_h24 and x_h40; it must accept R_b itself and R_b with every stored
value moved by one bf16 ulp at random. No GPU: the backward oracle, teacher-forced on the device's saved
tensors in the GPU test, is teacher-forced on the forward R_b here.

The default seeds (sum of the code points of "case-cell") were checked to satisfy all of this; SEED in the
helper overrides one if a later change to the table needs it."""
import pytest
import torch

import _rnn_cases as C

MUTATION_CASES = ("h8", "b33_h24", "x_h40")
CELLS_OF = {
    "tf_gates_in_cudnn_order": (C.LSTM_TF,),
    "no_forget_bias": (C.LSTM_TF,),
    "gru_bias_outside_r": (C.GRU,),
    "reverse_from_T": C.ALL3,
    "dgr_is_dgx": (C.GRU,),
    "no_dhz_carry_unit": (C.GRU,),
    "no_dc_carry_step": (C.LSTM_CUDNN, C.LSTM_TF),
}
MUTANTS = [(m, case, cell) for m in C.FWD_MUTATIONS + C.BWD_MUTATIONS for case in MUTATION_CASES
           for cell in CELLS_OF[m] if cell in C.spec(case)["cells"]]


def _quiet(*a):
  pass


def _oracle_result(case, cell, fwd_mutate=None, bwd_mutate=None):
  """(got, R_b): the rounded oracle with the given mutation, and the unmutated R_b teacher-forced on got's own
  saved tensors, as the GPU test does with the device's."""
  d = C.build_inputs(case, cell)
  s = C.spec(case)
  xcd = C.paths(case, cell)[1] == "xcd"
  if fwd_mutate is None:
    fw = C.reference_fwd(case, cell, True)
  else:
    fw = [C.forward_oracle(cell, x["gx"], x["wh"], x["bh"], d["lens"], x["reverse"], rounded=True, mutate=fwd_mutate)
          for x in d["dirs"]]
  at = s["H"] // 2 + 1 if bwd_mutate == "no_dhz_carry_unit" else 1
  bw = [C.backward_oracle(cell, f["gates"], f.get("c_seq"), f["y"], x["dy"], x["wh"], d["lens"], x["reverse"],
                          rounded=True, xcd=xcd, mutate=bwd_mutate, mutate_at=at) for x, f in zip(d["dirs"], fw)]
  got = [dict(f, **b) for f, b in zip(fw, bw)]
  Rb = [dict(f, **b) for f, b in zip(C.reference_fwd(case, cell, True), C.reference_bwd(case, cell, fw, True))]
  return got, Rb


@pytest.mark.parametrize("case,cell", C.RUNS, ids=["%s-%s" % r for r in C.RUNS])
def test_inputs_and_accepts_rb_cpu(case, cell):
  """Input sanity (lengths within [0, T + 3] and containing 1 and T; the mean |2 s - 1| of the two sigmoid
  gates r, z / i, f below 0.99: not saturated) and compare() accepts R_b."""
  bad = C.check_inputs(case, cell)
  assert not bad, "\n".join(bad)
  got, Rb = _oracle_result(case, cell)
  fails = C.compare(case, cell, got, Rb, C.noise_floor(), log=_quiet)
  assert not fails, "\n".join(fails)


def test_noise_floor_cpu():
  """n_q is a bf16 rounding effect: above zero, and far below the values it bounds."""
  nq = C.noise_floor()
  print("n_q", nq)
  for cell in C.ALL3:
    for q in C.outputs_of(cell):
      assert 0.0 < nq[cell][q] < 0.05, (cell, q, nq[cell][q])


@pytest.mark.parametrize("case", MUTATION_CASES)
def test_accepts_one_ulp_moves_cpu(case):
  """Every stored value of R_b moved by one bf16 ulp up or down at random (c_seq, stored as fp32, by 2^-9 of
  its value): compare() still accepts. Zeros stay: rows of finished steps must be exact."""
  for cell in C.spec(case)["cells"]:
    got, Rb = _oracle_result(case, cell)
    g = torch.Generator().manual_seed(11)
    moved = []
    for r in got:
      m = {}
      for q, t in r.items():
        sign = torch.randint(0, 2, t.shape, generator=g) * 2 - 1
        if q == "c_seq":
          m[q] = t * (1.0 + sign * 2.0 ** -9)
        else:
          b16 = t.to(torch.bfloat16)
          assert torch.equal(b16.double(), t), q           # R_b holds bf16 values there
          bits = b16.view(torch.int16) + torch.where(t != 0, sign, torch.zeros_like(sign)).to(torch.int16)
          m[q] = bits.view(torch.bfloat16).double()
          assert bool(((m[q] - t).abs() > 0).eq(t != 0).all())
      moved.append(m)
    fails = C.compare(case, cell, moved, Rb, C.noise_floor(), log=_quiet)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("mutation,case,cell", MUTANTS, ids=["%s-%s-%s" % m for m in MUTANTS])
def test_rejects_wrong_recurrence_cpu(mutation, case, cell):
  fwd = mutation if mutation in C.FWD_MUTATIONS else None
  bwd = mutation if mutation in C.BWD_MUTATIONS else None
  got, Rb = _oracle_result(case, cell, fwd, bwd)
  fails = C.compare(case, cell, got, Rb, C.noise_floor(), log=_quiet)
  assert fails, "compare() accepted the mutation %s on %s-%s" % (mutation, case, cell)
  # the mutation must be caught where it acts: a forward one on a forward output, a backward one on dgx / dgr
  where = ("y", "gates", "c_seq") if fwd else ("dgx", "dgr")
  assert any((" %s " % q) in f for f in fails for q in where), fails
