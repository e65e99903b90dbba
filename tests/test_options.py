"""CPU tests of the library's option registry (they need the built library, as test_boundary.py does): the
registry's getenv is the only one of the library, every option reads back what was set, and each OS2S_*
variable a registration names lands in its option when the library is loaded. No test here makes a GPU call."""
import ctypes
import glob
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Written out by hand from the issue's table, not derived from the library:
# variable -> (option, default, a non-default text, the value that text maps to)
ENV = {
    "OS2S_DETERMINISTIC": ("deterministic", 0, "1", 1),
    "OS2S_PP_MIN_COUT": ("conv1d.pp_min_cout", 320, "384", 384),
    "OS2S_WGRAD_PP_MIN_UNITS": ("conv1d_wgrad.pp_min_units", 8, "12", 12),
    "OS2S_WGRAD1X1_PP": ("conv1d_wgrad.k1_pp", -1, "0", 0),
    "OS2S_SKINNY_VARIANT": ("gemm_skinny.variant", -1, "l32", 1),
    "OS2S_CTC_WAVE": ("ctc_loss.wave", 1, "0", 0),
    "OS2S_GRU_XCD": ("gru_xcd.fwd", 1, "0", 0),
    "OS2S_GRU_XCD_BWD": ("gru_xcd.bwd", 1, "0", 0),
    "OS2S_ATTN_SPLIT": ("attn_decoder.attn_split", 1, "0", 0),
    "OS2S_CELL_SPLIT": ("attn_decoder.cell_split", 1, "0", 0),
    "OS2S_AD_FAST": ("attn_decoder.fast", 1, "0", 0),
    "OS2S_TI_ROWS": ("tacotron_infer.rows", 16, "32", 32),
    "OS2S_TI_GEOM": ("tacotron_infer.geom", 0, "9x4", 904),
    "OS2S_TI_CTX_PARTS": ("tacotron_infer.ctx_parts", 0, "2", 2),
    "OS2S_TI_DEBUG": ("tacotron_infer.debug", 0, "3", 3),
}
# the options no variable feeds, with their defaults
PLAIN = {
    "conv1d.variant": -1, "conv1d.split": -1, "conv1d.pp_cost_256": 1.19, "conv1d.pp_cost_2x128": 0.90,
    "conv1d.pp_cost_3x128": 1.06, "conv1d.pp_dgrad_penalty": 1000, "conv1d.pp_prio": 0, "conv1x1.variant": -1,
    "conv1x1.order": 1, "conv1d_wgrad.variant": -1, "conv1d_wgrad.split": -1, "conv1d_wgrad.sw_ablate": 0,
    "conv1d_wgrad.xcd_order": 1, "gemm_nt.split": -1, "gemm_nt.tile": 0, "depthwise.variant": -1,
    "depthwise.ablate": 0, "bn.act_fwd.groups": 32, "bn.act_fwd.rows": 32, "bn.act_bwd_reduce.groups": 32,
    "bn.act_bwd_reduce.rows": 64, "bn.bwd_apply.groups": 32, "bn.bwd_apply.rows": 64,
}
UNKNOWN = "no.such.option"

CHILD = ("import json; from openseq2seq_amd import _lib; "
         "print('OPTIONS ' + json.dumps({n: _lib.get_option(n) for n in _lib.option_names()}))")


def _child_options(variables):
  """get_option of every name in a fresh interpreter that only loads the library, started with `variables`."""
  env = {k: v for k, v in os.environ.items() if k not in ENV}
  env.update(variables)
  r = subprocess.run([sys.executable, "-c", CHILD], env=env, cwd=REPO, timeout=300, stdout=subprocess.PIPE,
                     stderr=subprocess.STDOUT, text=True)
  assert r.returncode == 0, r.stdout[-4000:]
  return json.loads([l for l in r.stdout.splitlines() if l.startswith("OPTIONS ")][-1][len("OPTIONS "):])


def test_one_getenv_in_the_library():
  hits = {}
  for ext in ("hip", "hpp", "cpp"):
    for f in glob.glob(os.path.join(REPO, "openseq2seq_amd", "csrc", "*." + ext)):
      n = open(f, errors="ignore").read().count("getenv(")
      if n:
        hits[os.path.basename(f)] = n
  assert hits == {"os2s_api.hip": 1}, hits


def test_every_option_reads_back_what_was_set():
  from openseq2seq_amd import _lib
  names = _lib.option_names()
  assert sorted(names) == sorted([v[0] for v in ENV.values()] + list(PLAIN))
  for n in names:
    old = _lib.get_option(n)
    try:
      for v in (16, 24):     # inside the range of every option that has one (bn.*: 8 .. 256 / 8 .. 1024)
        _lib.set_option(n, v)
        assert _lib.get_option(n) == v, n
    finally:
      _lib.set_option(n, old)
    assert _lib.get_option(n) == old, n
  g = _lib.bind("os2s_get_option", [ctypes.c_char_p, ctypes.POINTER(ctypes.c_double)])
  v = ctypes.c_double(7.0)
  assert g(UNKNOWN.encode(), ctypes.byref(v)) == -1 and g(None, ctypes.byref(v)) == -1 and v.value == 7.0
  assert g(b"conv1d.pp_prio", None) == -1
  assert g(b"conv1d.pp_prio", ctypes.byref(v)) == 0 and v.value == _lib.get_option("conv1d.pp_prio")
  with pytest.raises(_lib.Os2sError):
    _lib.get_option(UNKNOWN)


def test_environment_reaches_the_options_at_load():
  got = _child_options({})
  want = dict(PLAIN)
  want.update({opt: default for opt, default, _, _ in ENV.values()})
  assert sorted(got) == sorted(want)
  for n, v in want.items():
    assert got[n] == pytest.approx(v, rel=1e-6), n
  got = _child_options({var: text for var, (_, _, text, _) in ENV.items()})
  for opt, _, _, mapped in ENV.values():
    assert got[opt] == mapped, opt
  for n, v in PLAIN.items():
    assert got[n] == pytest.approx(v, rel=1e-6), n
  got = _child_options({"OS2S_SKINNY_VARIANT": "wide"})
  assert got["gemm_skinny.variant"] == 3
  assert all(got[opt] == default for opt, default, _, _ in ENV.values() if opt != "gemm_skinny.variant")


def test_entry_points_work_on_the_registered_variables():
  from openseq2seq_amd import _lib
  old = _lib.C.os2s_deterministic()
  try:
    for on in (1, 0):
      _lib.C.os2s_set_deterministic(on)
      assert _lib.get_option("deterministic") == on and _lib.C.os2s_deterministic() == on
    _lib.set_option("deterministic", 1)
    assert _lib.C.os2s_deterministic() == 1
  finally:
    _lib.C.os2s_set_deterministic(old)
  fwd = _lib.get_option("gru_xcd.fwd")
  try:
    for mode in (0, -1):
      _lib.C.os2s_gru_xcd_set_mode(mode)
      assert _lib.get_option("gru_xcd.fwd") == fwd
  finally:
    _lib.C.os2s_gru_xcd_set_mode(-1)
