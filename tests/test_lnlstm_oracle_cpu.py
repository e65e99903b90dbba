"""The float64 oracle of tests/_lnlstm_cases.py, on the CPU.

* The backward oracle is the gradient of the forward oracle: torch.autograd of the plain forward (R) with respect
  to gx and ln against backward_oracle() teacher-forced on R's own saved tensors, to float64 round-off.
* The host restatement of the dropout counter hash keeps about `keep` of the elements and is a function of
  (seed, index) alone.
* The bound can fail: within() is fed, in place of a device result, the output of a deliberately wrong float64
  recurrence (rounded like R_b, so the mutation is the only difference) and must reject every one of the eight;
  it must accept R_b itself."""
import pytest
import torch

import _lnlstm_cases as C

SMALL = [c for c in C.CASES if C.spec(c)["B"] * C.spec(c)["H"] <= 4096]
# the case a mutation is shown on: the dropout ones need keep < 1, the rest ragged lengths and several steps
MUTATION_CASE = {m: ("keep07_h40" if m in ("no_keep_scale", "mask_by_live_row") else "b33_h24") for m in C.MUTATIONS}


@pytest.mark.parametrize("case", SMALL)
def test_backward_oracle_is_the_gradient_cpu(case):
  d = C.build_inputs(case)
  gx = d["gx"].double().requires_grad_(True)
  ln = d["ln"].double().requires_grad_(True)
  fw = C.forward_oracle(gx, d["wh"], ln, d["lens"], d["mask"], d["keep"], d["h0"], d["c0"])
  (fw["y"] * d["dy"].double()).sum().backward()
  saved = {k: v.detach() for k, v in fw.items()}
  bw = C.reference_bwd(case, saved, False)
  for got, ref, what in ((bw["dgx"], gx.grad, "dgx"), (bw["dln"], ln.grad, "dln")):
    scale = float(ref.abs().max())
    assert scale > 0.0
    assert float((got - ref).abs().max()) <= 1e-11 * scale, what


def test_host_mask_cpu():
  m = C.host_mask(1234, 1 << 16, 0.7)
  assert abs(float(m.double().mean()) - 0.7) < 0.01
  assert torch.equal(m[:4096], C.host_mask(1234, 4096, 0.7))
  assert not torch.equal(m[:4096], C.host_mask(1235, 4096, 0.7))
  assert bool(C.host_mask(7, 4096, 1.0).all())


@pytest.mark.parametrize("case", list(C.CASES))
def test_bound_accepts_rb_cpu(case):
  Rb = C.reference_fwd(case, True)
  got = dict(Rb, **C.reference_bwd(case, Rb, True))
  nq = C.noise_floor(case)
  assert all(ok for _, ok, _, _ in C.within(case, got, got, nq))
  s = C.spec(case)
  if s["T"] > 1:
    assert nq["y"] > 0.0 and nq["xhat"] > 0.0 and nq["dgx"] > 0.0 and nq["s_hat"] > 0.0


@pytest.mark.parametrize("mutation", C.MUTATIONS)
def test_bound_rejects_wrong_recurrence_cpu(mutation):
  case = MUTATION_CASE[mutation]
  d = C.build_inputs(case)
  with torch.no_grad():
    fw = C.forward_oracle(d["gx"], d["wh"], d["ln"], d["lens"], d["mask"], d["keep"], d["h0"], d["c0"], rounded=True,
                          mutate=mutation)
  got = {k: fw[k] for k in C.FWD_OUT}
  res = C.within(case, got, C.reference_fwd(case, True), C.noise_floor(case))
  assert not all(ok for _, ok, _, _ in res), "the bound accepts the mutation %s" % mutation
  assert not dict((q, ok) for q, ok, _, _ in res)["y"], "y alone does not show the mutation %s" % mutation
