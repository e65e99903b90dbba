"""The float64 oracles of tests/_textcls_cases.py, on the CPU.

* The state-gradient backward oracle is the gradient of _lnlstm_cases.forward_oracle: autograd of
  sum y dy + sum hT dhT + sum cT dcT with respect to gx and ln against backward_state_oracle() teacher-forced on
  the forward's own saved tensors, to float64 round-off (the tolerance of tests/test_lnlstm_oracle_cpu.py).
* The head oracle is the gradient of its own forward and loss under torch.autograd.
* The device bounds can fail: fed the output of a deliberately wrong oracle in place of a device result, they
  reject each of the five mutations on at least one case, and accept the oracle itself."""
import pytest
import torch

import _lnlstm_cases as C
import _textcls_cases as X

SMALL = [c for c in X.STATE_CASES if C.spec(c)["B"] * C.spec(c)["H"] <= 4096]


@pytest.mark.parametrize("mix", list(X.MIXES))
@pytest.mark.parametrize("case", SMALL)
def test_state_backward_oracle_is_the_gradient_cpu(case, mix):
  d = C.build_inputs(case)
  dy, dhT, dcT = X.mix_inputs(case, mix)
  gx = d["gx"].double().requires_grad_(True)
  ln = d["ln"].double().requires_grad_(True)
  fw = C.forward_oracle(gx, d["wh"], ln, d["lens"], d["mask"], d["keep"], d["h0"], d["c0"])
  obj = sum((fw[k] * g.double()).sum() for k, g in (("y", dy), ("hT", dhT), ("cT", dcT)) if g is not None)
  obj.backward()
  saved = {k: v.detach() for k, v in fw.items()}
  bw = X.reference_state_bwd(case, mix, saved, False)
  for got, ref, what in ((bw["dgx"], gx.grad, "dgx"), (bw["dln"], ln.grad, "dln")):
    scale = float(ref.abs().max())
    assert scale > 0.0
    assert float((got - ref).abs().max()) <= 1e-11 * scale, what


def test_state_oracle_without_state_gradient_is_the_plain_oracle_cpu():
  case = "b33_h24"
  Rb = C.reference_fwd(case, True)
  d = C.build_inputs(case)
  with torch.no_grad():
    a = X.backward_state_oracle(Rb["xhat"], Rb["s_hat"], Rb["rstd"], d["dy"], None, None, d["wh"], d["ln"], d["lens"],
                                rounded=True)
  b = C.reference_bwd(case, Rb, True)
  assert torch.equal(a["dgx"], b["dgx"]) and torch.equal(a["dln"], b["dln"])


@pytest.mark.parametrize("mutation", X.STATE_MUTATIONS)
def test_state_bound_rejects_mutation_cpu(mutation):
  rejected = []
  for case in ("h8", "b33_h24"):
    Rb = C.reference_fwd(case, True)
    for mix in X.MIXES:
      ref = X.reference_state_bwd(case, mix, Rb, True)
      nq = X.state_noise_floor(case, mix)
      assert all(ok for _, ok, _, _ in C.within(case, ref, ref, nq))
      got = X.reference_state_bwd(case, mix, Rb, True, mutate=mutation)
      if not all(ok for _, ok, _, _ in C.within(case, got, ref, nq)):
        rejected.append((case, mix))
  assert rejected, "the bound accepts the mutation %s on every case" % mutation


@pytest.mark.parametrize("case", list(X.HEAD_CASES))
def test_head_oracle_is_the_gradient_cpu(case):
  d = X.head_inputs(case)
  scale = 1024.0
  h = d["h"].double().requires_grad_(True)
  c = d["c"].double().requires_grad_(True) if d["c"] is not None else None
  w = d["w"].double().requires_grad_(True)
  bias = d["bias"].double().requires_grad_(True)
  s = h if c is None else torch.cat([h, c], dim=1)
  logits = s @ w.t() + bias
  logits.retain_grad()
  loss = -(torch.log_softmax(logits, dim=1) * d["y"].double()).sum() / d["B"]
  (loss * scale).backward()
  lo = X.head_fwd_oracle(d["h"], d["c"], d["w"], d["bias"])[0]
  x = X.xent_oracle(lo, d["y"], scale)
  b = X.head_bwd_oracle(d["h"], d["c"], d["w"], x["dlogits"][0], torch.zeros_like(d["g0w"]), torch.zeros_like(d["g0b"]))
  sgrad = h.grad if c is None else torch.cat([h.grad, c.grad], dim=1)
  for got, ref, what in ((lo, logits.detach(), "logits"), (x["loss"][0], loss.detach(), "loss"),
                         (x["dlogits"][0], logits.grad, "dlogits"), (b["dw"][0], w.grad, "dw"),
                         (b["dbias"][0], bias.grad, "dbias"), (b["ds"][0], sgrad, "ds")):
    tol = 1e-12 * max(float(ref.abs().max()), 1e-30)
    assert float((got - ref).abs().max()) <= tol, what


@pytest.mark.parametrize("mutation", X.HEAD_MUTATIONS)
def test_head_bound_rejects_mutation_cpu(mutation):
  rejected = []
  for case in X.HEAD_CASES:
    d = X.head_inputs(case)
    lo = X.head_fwd_oracle(d["h"], d["c"], d["w"], d["bias"])
    x = X.xent_oracle(lo[0], d["y"])
    assert X.head_within(lo[0].float(), lo, "logits")[0] and X.head_within(x["loss"][0].float(), x["loss"], "loss")[0]
    if mutation == "c_then_h":
      ok = X.head_within(X.head_fwd_oracle(d["h"], d["c"], d["w"], d["bias"], mutate=mutation)[0].float(), lo, "logits")[0]
    else:
      ok = X.head_within(X.xent_oracle(lo[0], d["y"], mutate=mutation)["loss"][0].float(), x["loss"], "loss")[0]
    if not ok:
      rejected.append(case)
  assert rejected, "the bound accepts the mutation %s on every case" % mutation
