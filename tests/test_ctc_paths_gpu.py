"""Every alpha / beta dispatch class of csrc/ctc_loss.hip, and the log-softmax, gradient and finish kernels beside
it, stage by stage against the float64 oracle of the stage's own inputs (tests/_ctc_cases.py: the case table, the
bounds and their derivations), then end to end against oracle.ctc.ctc_loss_torch. The workspace and the outputs
are prefilled with 0xFF bytes and sit between guard bytes that must keep their value; logits past in_len are NaN.
Each test prints its largest error / bound per stage
(CTC-RATIO lines)."""
import contextlib

import pytest
import torch

import _ctc_cases as cc

pytestmark = pytest.mark.gpu

GUARD = 4096


@contextlib.contextmanager
def wave(on):
  """The option ctc_loss.wave; the default comes back whatever happens."""
  from openseq2seq_amd import _lib
  _lib.set_option("ctc_loss.wave", on)
  try:
    yield
  finally:
    _lib.set_option("ctc_loss.wave", 1)


class Device:
  """The backend of _ctc_cases.check_case on the GPU: CPU tensors in, CPU tensors out."""

  def __init__(self, dev):
    self.dev, self.fails, self.guards = dev, [], []

  def filled(self, what, shape, dtype):
    """0xFF bytes viewed as `dtype`, GUARD more of them on either side."""
    n = torch.empty((), dtype=dtype).element_size()
    for d in shape:
      n *= d
    raw = torch.full((GUARD + n + GUARD,), 255, dtype=torch.uint8, device=self.dev)
    self.guards.append((what, raw, n))
    return raw[GUARD:GUARD + n].view(dtype).view(shape)

  def check_guards(self):
    for what, raw, n in self.guards:
      if not (bool((raw[:GUARD] == 255).all()) and bool((raw[GUARD + n:] == 255).all())):
        self.fails.append("%s: a guard byte was overwritten" % what)
    self.guards = []

  def run(self, inp):
    from openseq2seq_amd import _lib, capi
    T, B, V, Lmax = inp["T"], inp["B"], inp["V"], inp["Lmax"]
    up = lambda t: None if t is None else t.contiguous().to(self.dev)
    ws = self.filled("workspace", (int(_lib.C.os2s_ctc_loss_workspace_bytes(T, B, V, Lmax)),), torch.uint8)
    out = dict(loss_per_sample=self.filled("loss_per_sample", (B,), torch.float32),
               loss_mean=self.filled("loss_mean", (1,), torch.float32),
               dlogits=self.filled("dlogits", (T, B, V), torch.float32),
               dlogits_bf16=self.filled("dlogits_bf16", (B, T, inp["vpad"]), torch.bfloat16))
    with wave(inp["wave"]):
      assert capi.ctc_loss_kernel_class(V, Lmax) == inp["klass"], (inp["case"], inp["variant"])
      res = capi.ctc_loss(up(inp["logits"]), up(inp["in_len"]), up(inp["labels"]), up(inp["label_len"]),
                          blank=inp["blank"], grad_scale=inp["grad_scale"], want_grad=inp["want_grad"],
                          want_grad_bf16=inp["want_bf16"], vpad=inp["vpad"], grad_scale_dev=up(inp["grad_scale_dev"]),
                          workspace=ws, out=out, want_workspace=True)
      torch.cuda.synchronize()
    for k in ("loss_per_sample", "loss_mean"):
      assert res[k] is out[k]
    assert (res["dlogits"] is out["dlogits"]) if inp["want_grad"] else res["dlogits"] is None
    R = {k: (None if v is None else v.cpu()) for k, v in res.items() if k != "workspace"}
    R.update({k: v.cpu().clone() for k, v in res["workspace"].items()})
    if not inp["want_grad"] and not bool((out["dlogits"].view(torch.int32) == -1).all()):
      self.fails.append("dlogits was written although no fp32 gradient was asked for")
    self.check_guards()
    return R


@pytest.mark.parametrize("case,variant", cc.PAIRS, ids=["%s-%s" % p for p in cc.PAIRS])
def test_case(cuda, case, variant):
  be = Device(cuda)
  res = cc.check_case(case, variant, be)
  assert not res["fails"] and not be.fails, "\n".join(res["fails"] + be.fails)


def test_every_class_is_reached(cuda):
  """The library's own query names the class of every table row; <8> and both routes to the 256-thread kernel
  (V > 32, S > 1024) are among them."""
  from openseq2seq_amd import capi
  got = {name: capi.ctc_loss_kernel_class(c["V"], c["Lmax"]) for name, c in cc.CASES.items()}
  assert got == {name: c["klass"] for name, c in cc.CASES.items()}
  assert got["w8_lo"] == got["w8_hi"] == 8 and got["t256_v33"] == 0 and got["t256_l512"] == 0
  for name, c in cc.CASES.items():
    assert capi.ctc_loss_kernel_class(c["V"], c["Lmax"]) == cc.kernel_class_mirror(c["V"], c["Lmax"]), name
    with wave(0):
      assert capi.ctc_loss_kernel_class(c["V"], c["Lmax"]) == 0, name


def test_lds_limit(cuda):
  """Lmax = 910 is refused before a launch (the gradient kernel would need 65,556 B of LDS), Lmax = 909 runs
  (the t256_max case)."""
  from openseq2seq_amd import _lib, capi
  assert capi.ctc_loss_kernel_class(29, 909) == 0 and capi.ctc_loss_kernel_class(29, 910) == -1
  T, B, V, Lmax = 8, 1, 29, 910
  logits = torch.zeros(T, B, V, device=cuda)
  i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=cuda)
  with pytest.raises(_lib.Os2sError, match="code %d" % -3):
    capi.ctc_loss(logits, i32([T]), torch.zeros(B, Lmax, dtype=torch.int32, device=cuda), i32([2]))
