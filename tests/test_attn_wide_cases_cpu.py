"""The case table of tests/_attn_wide_cases.py, judged with the float64 oracle alone (no device): every
compared reference gradient is non-zero, the largest alignment weight is below 0.99, every sample has a live
step, and the bf16-store emulation R_b stays inside compare()'s forward tolerances against R, so that the
device comparison of tests/test_attn_decoder_wide_gpu.py has room left for the kernels' own error."""
import pytest

import _attn_decoder_cases as C
import _attn_wide_cases as W

EXISTING = dict(C.CASES)


@pytest.mark.parametrize("case", sorted(W.WIDE_CASES) + sorted(W.AB_CASES))
def test_wide_inputs_cpu(case):
  bad = W.check_inputs(case)
  assert not bad, "\n".join(bad)
  d = W.build_inputs(case)
  row = W.ALL[case]
  assert 1 in d["src_len"].tolist() and row[2] in d["src_len"].tolist()
  if d["tgt_len"] is not None:
    assert 1 in d["tgt_len"].tolist() and row[1] in d["tgt_len"].tolist()
  top = float(W.reference(case)["align"][d["src_len"] > 1].max())
  print("largest alignment weight %.4f" % top)


@pytest.mark.parametrize("case", sorted(W.WIDE_CASES))
def test_wide_rounded_forward_inside_bounds_cpu(case):
  bad = W.forward_within_compare_bounds(case)
  print("max|R_b - R|", W.own_distance(case))
  assert not bad, "\n".join(bad)


def test_existing_table_untouched_cpu():
  """The wide table lives in the existing module only inside installed()."""
  with W.installed():
    assert "gnmt_u1024" in C.CASES and "gnmt_u200" in C.TIGHT
  assert C.CASES == EXISTING and not set(W.ALL) & set(C.CASES)
  assert not set(W.WIDE_TIGHT) & set(C.TIGHT) and not set(W.WIDE_V_SCALE) & set(C.V_SCALE)
