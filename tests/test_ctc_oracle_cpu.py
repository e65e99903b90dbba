"""CPU proof that the bounds of tests/_ctc_cases.py are neither too tight nor unable to fail: check_case() accepts
the fp32 torch emulation of the algorithm of csrc/ctc_loss.hip on every case and variant, the same emulation in
float64 agrees with both CTC oracles, ten wrong backends each break a bound, and the library's two host queries
(kernel class, workspace layout) agree with the mirror of the dispatch and the workspace size. No GPU."""
import numpy as np
import pytest
import torch

import _ctc_cases as cc
from oracle import ctc


@pytest.mark.parametrize("case,variant", cc.PAIRS, ids=["%s-%s" % p for p in cc.PAIRS])
def test_fp32_emulation_keeps_every_bound(case, variant):
  res = cc.check_case(case, variant, cc.Emu())
  assert not res["fails"], "\n".join(res["fails"])


@pytest.mark.parametrize("case,variant", [(c, "base") for c in cc.CASES] + [(c, "blank0") for c in cc.VARIANTS["blank0"]],
                         ids=lambda v: v)
def test_fp64_emulation_agrees_with_the_oracles(case, variant):
  """The algorithm (renormalisation every 8th step, normaliser beside the rows, finite sentinel) computes what
  torch.nn.functional.ctc_loss and the direct numpy recursion compute: 1e-9 relative to max(1, |loss|), the
  gradient 1e-9 absolute."""
  inp = cc.make_inputs(case, variant)
  G = cc.geometry(inp)
  R = cc.Emu(cc.F64).run(inp)
  ref_loss, ref_grad = cc.reference(case, variant)
  tol = 1e-9 * ref_loss.abs().clamp_min(1.0)
  assert bool(((R["loss_per_sample"] - ref_loss).abs() <= tol).all()), (R["loss_per_sample"], ref_loss)
  assert float((R["dlogits"] - ref_grad).abs().max()) <= 1e-9
  assert torch.equal(R["valid"] != 0, inp["feasible"])
  if inp["T"] * G["Smax"] * inp["B"] < 3e5:
    ref = ctc.ctc_loss_numpy(inp["clean"].numpy(), G["Tb"].numpy(), inp["labels"].numpy(), G["L"].numpy(),
                             blank=inp["blank"])
    assert np.all(np.abs(R["loss_per_sample"].numpy() - ref) <= tol.numpy()), (R["loss_per_sample"], ref)


def test_dispatch_mirror_agrees_with_the_table():
  for name, c in cc.CASES.items():
    assert cc.kernel_class_mirror(c["V"], c["Lmax"]) == c["klass"], name
    assert cc.kernel_class_mirror(c["V"], c["Lmax"], wave=0) == 0, name
  for V, Lmax, k in ((29, 0, 4), (29, 127, 4), (29, 128, 8), (29, 255, 8), (29, 256, 16), (29, 511, 16), (29, 512, 0),
                     (32, 12, 4), (33, 12, 0), (29, 909, 0), (29, 910, -1), (40, 909, 0)):
    assert cc.kernel_class_mirror(V, Lmax) == k, (V, Lmax)
  assert sorted(set(c["klass"] for c in cc.CASES.values())) == [0, 4, 8, 16]


@pytest.mark.parametrize("mutant", list(cc.MUTANTS))
def test_wrong_backend_breaks_a_bound(mutant):
  res = cc.check_case(cc.MUTANTS[mutant], "base", cc.Emu(mutant=mutant), log=lambda line: None)
  assert res["fails"], "%s passes every stage" % mutant


def test_library_queries_agree_with_the_mirror_and_the_workspace_size():
  """The two host queries need no device: os2s_ctc_loss_kernel_class against the mirror on both sides of every
  threshold under both values of ctc_loss.wave, os2s_ctc_loss_workspace_layout against the sizes of the sections
  and os2s_ctc_loss_workspace_bytes."""
  import ctypes
  from openseq2seq_amd import _lib, capi
  for on in (1, 0):
    _lib.set_option("ctc_loss.wave", on)
    try:
      for V in (2, 5, 29, 32, 33, 40):
        for Lmax in (0, 1, 127, 128, 255, 256, 511, 512, 909, 910, 5000):
          assert capi.ctc_loss_kernel_class(V, Lmax) == cc.kernel_class_mirror(V, Lmax, on), (V, Lmax, on)
    finally:
      _lib.set_option("ctc_loss.wave", 1)
  assert capi.ctc_loss_kernel_class(1, 10) == -1 and capi.ctc_loss_kernel_class(29, -1) == -1
  lay = (ctypes.c_longlong * 8)()
  for c in list(cc.CASES.values()) + [dict(T=1, V=2, Lmax=0, samples=[0])]:
    T, B, V, Lmax = c["T"], len(c["samples"]), c["V"], c["Lmax"]
    assert _lib.C.os2s_ctc_loss_workspace_layout(T, B, V, Lmax, lay) == 0
    off, Sld = list(lay)[:7], int(lay[7])
    assert Sld == (2 * Lmax + 1 + 15) // 16 * 16
    need = [B * T * V * 4, B * T * Sld * 4, B * T * Sld * 4, B * T * 8, B * T * 8, B * 8, B * 4]
    assert off[0] == 0 and all(o % 256 == 0 for o in off[:6]) and off[6] % 4 == 0
    for i in range(6):
      assert off[i] + need[i] <= off[i + 1], (i, off, need)
    assert off[6] + need[6] + 255 <= int(_lib.C.os2s_ctc_loss_workspace_bytes(T, B, V, Lmax))     # + the alignment slack
  assert _lib.C.os2s_ctc_loss_workspace_layout(0, 1, 29, 4, lay) == -1
  assert _lib.C.os2s_ctc_loss_workspace_layout(8, 1, 29, 4, None) == -1
