"""Helper of tests/test_attn_decoder_wide_gpu.py and tests/test_attn_wide_cases_cpu.py (not a test module):
the attention-decoder cases beyond the old kernel limits (U % 128 == 0, U <= 512, all keys of a sample in
LDS). It reuses build_inputs / reference / run_gpu / compare / check_inputs / noise_floor of
tests/_attn_decoder_cases.py, which look their shapes up in that module's CASES / V_SCALE / TIGHT: the wide
table is installed there only while one of the functions below runs (installed()), never at import, so the
existing test keeps parametrising over its own table.

Columns as in the existing table: B, T, S, L, H, M, U, mode, K, F, use_bias, attn_in_keep, out_keep, ragged.

LDS footprints (attn_lds_floats, 160 KB = 40960 floats) say which residency each pass of a case takes:
  gnmt_u1024, bahd_u1024_l2, luong_h1024, gnmt_u640, gnmt_u200, bahd_u8,
  luong_h128_s400 (25600 floats of keys: it fits)                           resident, forward and backward
  gnmt_u512_s200, gnmt_u1024_s96_l2, bahd_u128_s700, luong_h128_s700        streamed, forward and backward
  gnmt_full_width (the en-de-gnmt-like shape)                               resident forward, streamed backward
The AB_CASES restate four shapes of the existing table (all resident) and name, with gnmt_u1024, a longer source
buffer at which the same shape streams in both passes: run_gpu_padded runs the same inputs with keys / values
zero-padded to that S (the source lengths stay), and since no kernel touches a position past src_len the two
runs must agree bit for bit — the two residencies do the same arithmetic in the same order."""
import contextlib
from unittest import mock

import torch

import _attn_decoder_cases as C

WIDE_CASES = {
    "gnmt_u1024": (5, 3, 13, 1, 64, 64, 1024, 1, 0, 0, False, 0.8, 1.0, True),
    "bahd_u1024_l2": (3, 2, 9, 2, 64, 64, 1024, 0, 0, 0, False, 1.0, 1.0, False),
    "luong_h1024": (2, 2, 7, 1, 1024, 64, 1024, 3, 0, 0, False, 1.0, 1.0, False),
    "gnmt_u640": (4, 2, 11, 1, 64, 64, 640, 1, 0, 0, False, 1.0, 1.0, False),
    "gnmt_u200": (4, 2, 11, 1, 64, 64, 200, 1, 0, 0, False, 1.0, 1.0, False),
    "bahd_u8": (3, 2, 6, 1, 64, 64, 8, 0, 0, 0, False, 1.0, 1.0, False),
    "gnmt_u512_s200": (3, 2, 200, 1, 64, 64, 512, 1, 0, 0, False, 1.0, 1.0, True),
    "gnmt_u1024_s96_l2": (3, 3, 96, 2, 64, 128, 1024, 1, 0, 0, False, 0.8, 0.9, True),
    "bahd_u128_s700": (2, 2, 700, 1, 64, 64, 128, 0, 0, 0, False, 1.0, 1.0, False),
    "luong_h128_s400": (2, 2, 400, 1, 128, 64, 128, 3, 0, 0, False, 1.0, 1.0, False),
    "luong_h128_s700": (2, 2, 700, 1, 128, 64, 128, 3, 0, 0, False, 1.0, 1.0, False),
    "gnmt_full_width": (4, 3, 50, 1, 1024, 1024, 1024, 1, 0, 0, False, 0.8, 1.0, True),
}
WIDE_V_SCALE = {"bahd_u1024_l2": 0.06, "bahd_u128_s700": 0.6}
# shapes of gnmt_u256_l2, bahd_u256_l2, luong_h256_l2 and tiny_h8_m8, restated (own names: own seeds, own caches)
AB_CASES = {
    "ab_gnmt_u256_l2": (5, 4, 13, 2, 64, 128, 256, 1, 0, 0, False, 0.8, 1.0, True),
    "ab_bahd_u256_l2": (33, 3, 13, 2, 64, 64, 256, 0, 0, 0, False, 1.0, 0.9, False),
    "ab_luong_h256_l2": (4, 3, 10, 2, 256, 64, 256, 3, 0, 0, False, 1.0, 1.0, True),
    "ab_tiny_h8_m8": (2, 2, 5, 1, 8, 8, 128, 0, 0, 0, False, 1.0, 1.0, False),
}
AB_V_SCALE = {"ab_bahd_u256_l2": 0.07}
# case -> S at which S * U / 2 floats of keys alone exceed the 40960 floats of LDS: streamed forward and backward
AB_STREAMED_S = {"ab_gnmt_u256_l2": 400, "ab_bahd_u256_l2": 400, "ab_luong_h256_l2": 400, "ab_tiny_h8_m8": 700,
                 "gnmt_u1024": 96}
# refused shapes: (case row, expected status)
REFUSED = {
    "refused_u1032": ((2, 1, 5, 1, 64, 64, 1032, 1, 0, 0, False, 1.0, 1.0, False), -1),
    "refused_u12": ((2, 1, 5, 1, 64, 64, 12, 1, 0, 0, False, 1.0, 1.0, False), -1),
    "refused_luong_u_ne_h": ((2, 1, 5, 1, 64, 64, 256, 3, 0, 0, False, 1.0, 1.0, False), -3),
    "refused_loc_u256": ((2, 1, 5, 1, 64, 64, 256, 2, 3, 2, False, 1.0, 1.0, False), -1),
}
ALL = dict(WIDE_CASES, **AB_CASES)
ALL.update({k: v[0] for k, v in REFUSED.items()})
WIDE_TIGHT = tuple(n for n in WIDE_CASES if WIDE_CASES[n][1] <= 2)
STRIDED = ISOLATION = STEPWISE = ("gnmt_u1024", "gnmt_u512_s200")
FWD_KEYS = ("y", "ctx", "align")


@contextlib.contextmanager
def installed():
  """The wide tables inside tests/_attn_decoder_cases.py for the duration of the block."""
  with mock.patch.dict(C.CASES, ALL), mock.patch.dict(C.V_SCALE, dict(WIDE_V_SCALE, **AB_V_SCALE)), \
       mock.patch.object(C, "TIGHT", C.TIGHT + WIDE_TIGHT):
    yield


def reference(name, **kw):
  with installed():
    return C.reference(name, **kw)


def build_inputs(name):
  with installed():
    return C.build_inputs(name)


def check_inputs(name):
  with installed():
    return C.check_inputs(name, C.reference(name))


def run_gpu(name, device, **kw):
  with installed():
    return C.run_gpu(name, device, **kw)


def own_distance(name, device=None):
  """max|R_b - R| of one case per forward quantity, from the oracle alone."""
  with installed():
    R, Rb = C.reference(name, device=device), C.reference(name, rounded=True, device=device)
  return {q: float((Rb[q] - R[q]).abs().max()) for q in FWD_KEYS}


def forward_within_compare_bounds(name):
  """R_b against R under compare()'s forward tolerances (y, ctx: atol = rtol = 3e-2; align: atol 5e-3,
  rtol 3e-2): the bf16 stores alone must not use them up. Returns the violations."""
  with installed():
    R, Rb = C.reference(name), C.reference(name, rounded=True)
  bad = []
  for q, atol, rtol in (("y", 3e-2, 3e-2), ("ctx", 3e-2, 3e-2), ("align", 5e-3, 3e-2)):
    err = (Rb[q] - R[q]).abs()
    if not bool((err <= atol + rtol * R[q].abs()).all()):
      bad.append("%s: R_b %s leaves compare()'s forward bound: max err %.3e" % (name, q, float(err.max())))
  return bad


def tight_nq(name, device=None, log=print):
  """n_q of the R_b bound for a wide T <= 2 case: the larger of the existing table's noise floor (computed
  on the existing table, before the wide one is installed) and the case's own max|R_b - R|."""
  base = C.noise_floor()
  own = own_distance(name, device)
  nq = {q: max(base[q], own[q]) for q in FWD_KEYS}
  log("  n_q %s: floor %s own %s -> used %s" % (name, base, own, nq))
  return nq


def check_case(name, device, log=print):
  """Device run and every assertion of compare(); T <= 2 cases also under the R_b bound. (got, failures)."""
  nq = tight_nq(name, device, log) if name in WIDE_TIGHT else None
  with installed():
    got, R = C.run_case(name, device)
    Rb = C.reference(name, rounded=True, device=device) if name in WIDE_TIGHT else None
    return got, C.compare(name, got, R, Rb, nq, log=log)


def compare_runs(name, a, b, keys, what, **kw):
  return C.compare_runs(name, a, b, keys, what, **kw)


def run_forward(name, device, stepwise):
  """Forward only through capi.AttnDecoder: one call over [0, T), or one call per step as greedy and beam
  decoding drive it. CPU tensors of y, ctx, align."""
  from openseq2seq_amd import capi
  with installed():
    B, T, S, L, H, M, U, mode, K, F, use_bias, a_keep, o_keep, ragged = C.CASES[name]
    d = C.build_inputs(name)
  todev = lambda t: None if t is None else t.to(device)
  dec = capi.AttnDecoder(B, T, S, L, H, M, U, mode, device, use_bias=use_bias, loc_k=K, loc_f=F, forget_bias=1.0,
                         attn_in_keep=a_keep, attn_in_seed=C.ATTN_IN_SEED, out_keep=o_keep, out_seeds=C.OUT_SEEDS)
  dec.set_params([w.to(device) for w in d["wcat"]], d["wq"].to(device), d["v"].to(device),
                 bias=[todev(b) for b in d["bias"]], g=todev(d["g"]), b=todev(d["b"]))
  dec.set_inputs(d["gx0"].to(device), d["keys"].to(device), d["values"].to(device), d["src_len"].to(device),
                 todev(d["tgt_len"]))
  if stepwise:
    for t in range(T):
      dec.forward(t, t + 1)
  else:
    dec.forward()
  return dict(y=dec.y_top.cpu(), ctx=dec.ctx.cpu(), align=dec.align_seq.cpu())


def run_gpu_padded(name, device, S_big):
  """run_gpu of a case's own inputs inside source buffers of S_big positions (keys / values zero past the case's S,
  as they are past src_len anyway; src_len unchanged)."""
  with installed():
    d, row = dict(C.build_inputs(name)), list(C.CASES[name])
  S = row[2]
  assert S_big > S and S_big * row[6] // 2 > 40960
  pad = lambda t: torch.cat([t, t.new_zeros((S_big - S,) + tuple(t.shape[1:]))], 0)
  for k in ("keys", "values"):
    d[k] = torch.stack([pad(t) for t in d[k]])
  row[2] = S_big
  big = "%s@s%d" % (name, S_big)
  with installed(), mock.patch.dict(C.CASES, {big: tuple(row)}), mock.patch.object(C, "build_inputs", lambda n: d):
    return C.run_gpu(big, device, second_backward=False)
