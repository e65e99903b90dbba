"""Helper of tests/test_depthwise_kernels_gpu.py and tests/test_depthwise_oracle_cpu.py (not a test module): the
case table that reaches every kernel and dispatch class of csrc/depthwise.hip, a pure-Python copy of the dispatcher's
class arithmetic, a float64 oracle per operation, the rounding bounds and compare().

Teacher forcing. x, dy, dz, addend, mask_ref and stat_ref are bf16 tensors made on the host, w and dw are fp32; the
oracle evaluates the header's formula in float64 on exactly those tensors. The two partial sums of the fused data
gradient are checked against float64 sums of the dx the backend itself stored. Every bound follows from
    u32 = 2^-24   unit roundoff of fp32          ubf = 2^-8   unit roundoff of bf16 round-to-nearest-even
(_bn_cases.py) and stands next to the code below; none was tuned on a device.

A backend (the device in test_depthwise_kernels_gpu.py, the fp32 torch emulations in test_depthwise_oracle_cpu.py)
gives, on CPU tensors,
    fwd(x, w, in_len, out_len, tout, stride, dil, pad_left, flip, variant) -> y bf16 [B, tout, C]
    wgrad(x, dy, dw0, in_len, stride, dil, pad_left, variant, det) -> dw fp32 [K, C] = dw0 + the gradient
    fused(dz, w, addend, alias, mask_ref, stat_ref, out_len, pad_left, mask_scale) -> dx, stats [nparts, 2, C]
        (alias: addend is handed over as the dx buffer itself)
Rows of x at t >= in_len[b] hold `poison` (NaN on the device) in every run with a length vector, and a rerun on
zeroed rows must give the same bits. With out_len only the rows t < out_len[b] of a forward are asserted; the fused
call must also leave +0 in every row t >= out_len[b] (mask_ref is zero there, dead tiles are zero-filled).

Classes reached (fwd_class / wgrad_class below are the dispatcher's arithmetic, re-derived from its formulas):
  forward / data gradient (flip 0 and 1)
    matrix cores    Jt = 3 .. 8 with K on both sides of every edge (2, 17|18, 33|34, 49|50, 65|66, 81|82, 96): tiles
                    of 992, 960 and 928 steps; Tout = tile - 1, tile, tile + 1, 2 tile + 5; padL = SAME, 0 (Tout =
                    Tin - K + 1) and K - 1 (Tout = Tin + K - 1); C = 8 (one group), 24, 32, 40 (second block, one live
                    group); the zero-fill of a tile whose input window lies past in_len (a later tile, and the first
                    one at padL = 0 with a length of 0; the register window too), the skip of a tile past out_len
                    (test_dead_tile_paths_are_reached asserts these from the table); a hi + lo case (init "split") whose result IS the lo table's contribution
    register window <1>: K = 1, 97, 257 by default, K = 2, 33, 96 under depthwise.variant 1; <2>: K = 39, 87; <4>:
                    K = 20, 64; Tout = 255, 256, 257, 299 (partial residue classes in the last 16-output block);
                    C up to 72 (second 64-channel block with one live group)
    generic         general loop: stride 2 (K = 11, 33), stride 3, dilation 3, stride 2 with dilation 2; register-blocked
                    branch under depthwise.variant 0: K = 2, 33, 75 with Tout = 127, 128, 129, 261; K = 233, the
                    largest whose tile fits 160 KB (K = 234 must raise and launch nothing)
  weight gradient (dw zero and non-zero on entry, deterministic mode twice)
    matrix cores    NT = 2 .. 7 with K on both sides of every edge; Tout = 927, 928, 929; Tout = 1900 (one workgroup
                    carries its accumulators over three tiles per sample in deterministic mode)
    register window <1>: K = 1 (nseg 8), 97 (2), 129, 256 (1); <2>: K = 39 (4), 87 (2); <4>: K = 20 (8), 64 (4)
    generic         by fall-through: dilation 4 K = 65 and dilation 2 K = 129 (nseg rounds to 0), K = 257 (more than 256
                    cells: general loop), dilation 3, stride 2; under variant 0 the register-blocked branch at K = 2, 33
                    (nseg 4), 75 (3), 129 (1); one launch per tile in deterministic mode; K = 313 | 314, the 160 KB edge
  fused data gradient
    one K per Jt class (11, 33, 39, 51, 75, 87); addend absent / separate / dx itself; mask_scale 1 and fl32(1 / 0.8);
    mask_ref a ReLU output with exact zeros inside live rows; C = 8, 40; Tout = 300, tile, 2 tile + 5; ragged out_len
    with dead tiles (their partials stay zero) and a 0; os2s_depthwise_dgrad_bnact_num_parts
Not reached: the 160 KB checks of the matrix-core forward and of the register-window weight gradient (no K the
dispatcher admits there exceeds 160 KB: 73 KB and at most 102 KB; the CPU test asserts that from the formulas); negative
padL; tensors of 2^31 bytes and more (a size changes no class: all row offsets are 64-bit); depthwise.ablate (a
measurement hook); pointwise_fold* (tests/test_sepconv_gpu.py).

Measured on the MI355X, largest error / bound over all cases (the GPU test prints them as DW-RATIO lines):
  forward / data gradient   y   matrix cores 0.991   register window 0.993   generic 0.995 (bf16 ties: ubf |ref| is
                                the rounding's own worst case); the hi + lo case 0.915, equal to the emulations
  weight gradient           dw  matrix cores 4.0e-4  register window 8.6e-3  generic 0.47 (the fp32 rounding of
                                dw0 + gradient at K = 257, where few terms make the bound small)
  fused data gradient       dx 0.957   stats[0] 8.1e-4   stats[1] 7.2e-3; +0 rows, +0 elements and dead tiles exact
No bound was widened: the matrix-core weight gradient sits four orders below n u32 sum|terms|, so whatever rounding an
MFMA applies inside its 32-product accumulation, the factor the issue allows for it stays 1 (MFMA_WGRAD_FACTOR). The
run found no wrong result in csrc/depthwise.hip or its bindings: the kernels are unchanged.
"""
import math
import os
import sys
import zlib

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
  sys.path.insert(0, REPO)

from _bn_cases import BF16, F32, F64, U32, UBF, _Checks, f32, live_rows   # noqa: E402

LDS_MAX = 160 * 1024
SPLIT_RESIDUAL = 2.0 ** -17


def ceil_div(a, b):
  return -(-a // b)


def same_padding(tin, k, stride, dil):
  tout = ceil_div(tin, stride)
  return tout, max((tout - 1) * stride + (k - 1) * dil + 1 - tin, 0) // 2


# ---------------------------------------------------------------------------------------------------------
# the dispatcher's class arithmetic (csrc/depthwise.hip: dm_geom, the three launchers), written out again
# ---------------------------------------------------------------------------------------------------------
def dm_geom(K):
  Jt = (32 + K - 1 + 15) // 16
  nseg = min((1056 - 16 * Jt) // 32, 32)
  nchunk = (32 * (nseg - 1) + 16 * Jt) // 8
  phys = (nchunk - 1) + ((nchunk - 1) >> 4) + 1
  while (phys * 16) % 256 != 128:
    phys += 1
  return dict(Jt=Jt, nseg=nseg, tile=32 * nseg, nchunk=nchunk, plane_bytes=phys * 16, wt=16 * Jt + 40)


def mfma_fwd_lds(K):
  g = dm_geom(K)
  return 32 * g["plane_bytes"] + 8 * 2 * g["wt"] * 2


def win_fwd_lds(K, dil):
  return (((256 + (K - 1) * dil) * 136 + 15) & ~15) + K * 64 * 4


def generic_rows(K, stride, dil):
  return 127 * stride + (K - 1) * dil + 1


def generic_fwd_lds(K, stride, dil):
  return (generic_rows(K, stride, dil) * 72 + K * 64) * 4


def generic_wgrad_lds(K, stride, dil):
  return (generic_rows(K, stride, dil) + 128) * 72 * 4


MFMA_WGRAD_LDS = 16 * (2432 + 2176)
MFMA_WGRAD_TILE = 928


def mfma_wgrad_nt(K):
  return (K + 15 + 15) // 16


def win_wgrad_geom(K, dil):
  """(ngrp, nseg, LDS bytes) of depthwise_wgrad16_kernel<dil>; nseg = 0: the launcher falls through."""
  ngrp = ceil_div(K, 16)
  ncell = ngrp * 16
  nseg = min(256 // ncell, 8)
  nseg = (nseg // dil) * dil
  tiles = (256 + 16 * ngrp * dil) * 136 + 256 * 128
  red = max(nseg, 1) * ncell * 64 * 4
  return ngrp, nseg, max(tiles, red)


def generic_wgrad_nseg(K):
  """Time segments of the register-blocked branch of depthwise_wgrad_kernel; None: more than 256 cells."""
  ncell = ceil_div(K, 8) * 8
  return None if ncell > 256 else max(1, min(256 // ncell, 4))


def fwd_class(K, stride, dil, variant=-1):
  if stride == 1 and dil == 1 and 2 <= K <= 96 and variant not in (0, 1) and mfma_fwd_lds(K) <= LDS_MAX:
    return ("mfma", dm_geom(K)["Jt"])
  if stride == 1 and dil in (1, 2, 4) and variant != 0 and win_fwd_lds(K, dil) <= LDS_MAX:
    return ("win", dil)
  if generic_fwd_lds(K, stride, dil) > LDS_MAX:
    return ("unsupported",)
  return ("generic", "blocked" if stride == 1 and dil == 1 else "loop")


def wgrad_class(K, stride, dil, variant=-1):
  """("mfma", NT) | ("win", dil, nseg) | ("generic", "blocked", nseg) | ("generic", "loop", why) | ("unsupported",)"""
  if stride == 1 and dil == 1 and 2 <= K <= 96 and variant not in (0, 1):
    return ("mfma", mfma_wgrad_nt(K))
  why = "stride" if stride != 1 else "dil%d" % dil
  if stride == 1 and dil in (1, 2, 4) and variant != 0:
    _, nseg, lds = win_wgrad_geom(K, dil)
    if nseg >= 1 and lds <= LDS_MAX:
      return ("win", dil, nseg)
    why = "nseg0" if dil > 1 else "cells"
  if generic_wgrad_lds(K, stride, dil) > LDS_MAX:
    return ("unsupported",)
  if stride == 1 and dil == 1:
    nseg = generic_wgrad_nseg(K)
    return ("generic", "blocked", nseg) if nseg is not None else ("generic", "loop", "cells")
  return ("generic", "loop", why)


def fwd_tile(cls, K):
  return {"mfma": dm_geom(K)["tile"], "win": 256, "generic": 128}[cls[0]]


def wgrad_tile(cls):
  return {"mfma": MFMA_WGRAD_TILE, "win": 256, "generic": 128}[cls[0]]


def wgrad_adds(cls, B, Tout, C, det):
  """Workgroups (launches in the generic kernel's deterministic mode) that add into one dw element."""
  if cls[0] == "mfma":       # gx of the launcher; ONE per channel block in deterministic mode
    return 1 if det else max(1, min(ceil_div(512, ceil_div(C, 16)), B * ceil_div(Tout, MFMA_WGRAD_TILE)))
  if cls[0] == "win":
    return 1 if det else min(B * ceil_div(Tout, 256), 64)
  return B * ceil_div(Tout, 128)


def num_parts(B, Tout, K):
  return B * ceil_div(Tout, dm_geom(K)["tile"])


# ---------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------
CASES = {}
MF_K = (2, 17, 18, 33, 34, 49, 50, 65, 66, 81, 82, 96)
FUSED_K = (11, 33, 39, 51, 75, 87)
UNSUPPORTED = {"fwd": dict(K=234, stride=1, dil=1, variant=0), "wgrad": dict(K=314, stride=1, dil=1, variant=-1)}


def _add(op, K, C, B, T, s=1, d=1, pad="same", flip=0, variant=-1, ragged=True, olen=False, init="randn", **kw):
  """T counts the OUTPUT rows (the tiles run over them); Tin follows from pad."""
  name = "%s_K%d_s%dd%d_C%d_B%d_T%d_%s" % (op, K, s, d, C, B, T, pad)
  name += ("_flip" if flip else "") + ("_v%d" % variant if variant >= 0 else "") + ("" if ragged else "_dense")
  name += ("_olen" if olen else "") + ("_" + init if init != "randn" else "") + "".join("_%s%s" % i for i in kw.items())
  assert name not in CASES, name
  CASES[name] = dict(op=op, K=K, C=C, B=B, T=T, s=s, d=d, pad=pad, flip=flip, variant=variant, ragged=ragged,
                     olen=olen, init=init, **kw)


def _build():
  Cs4, Cs5, pads = (8, 24, 32, 40), (8, 24, 32, 40, 72), ("same", "valid", "full")
  # ---- forward, matrix cores: two cases per K; (C, T) run through all 16 pairs, (C, pad) through all 12
  for i, K in enumerate(MF_K):
    Tt = dm_geom(K)["tile"]
    for j in range(2):
      n = 2 * i + j
      _add("fwd", K, Cs4[n % 4], (3, 4, 2)[(n // 2) % 3], (Tt - 1, Tt, Tt + 1, 2 * Tt + 5)[(n + n // 4) % 4],
           pad=pads[n % 3], flip=(n + n // 8) % 2, ragged=n % 6 != 5, olen=(n // 3) % 2 == 1)
  _add("fwd", 50, 8, 3, dm_geom(50)["tile"] + 1, init="split")
  _add("fwd", 33, 24, 5, 2 * dm_geom(33)["tile"] + 5, flip=1, olen=True)
  # padL = 0 and a sample of length 0 without out_len: the FIRST tile's window lies past the end (zero-fill at t0 = 0)
  _add("fwd", 18, 8, 4, dm_geom(18)["tile"] + 1, pad="valid")
  _add("fwd", 97, 24, 4, 257, pad="valid", flip=1)
  # ---- forward, register window
  win = [(1, 1, -1), (97, 1, -1), (257, 1, -1), (2, 1, 1), (33, 1, 1), (96, 1, 1), (39, 2, -1), (87, 2, -1),
         (20, 4, -1), (64, 4, -1)]
  for i, (K, d, v) in enumerate(win):
    for j in range(2):
      n = 2 * i + j
      pad = "full" if n % 3 == 2 and (K - 1) * d < 100 else "valid" if n % 3 == 1 else "same"
      _add("fwd", K, Cs5[n % 5], (2, 3, 4)[n % 3], (255, 256, 257, 299)[(n + n // 4) % 4], d=d, pad=pad, flip=(n // 2) % 2,
           variant=v, ragged=n % 7 != 6, olen=n % 4 == 1)
  # ---- forward, generic
  gen = [(11, 2, 1, -1), (33, 2, 1, -1), (5, 3, 1, -1), (7, 1, 3, -1), (9, 2, 2, -1), (2, 1, 1, 0), (33, 1, 1, 0),
         (75, 1, 1, 0)]
  for i, (K, s, d, v) in enumerate(gen):
    for j in range(2):
      n = 2 * i + j
      _add("fwd", K, Cs5[n % 5], (4, 2, 3)[n % 3], (127, 129, 261, 128)[(n + n // 4) % 4], s=s, d=d,
           pad="valid" if n % 3 == 1 else "same", flip=(n // 2) % 2, variant=v, ragged=n % 7 != 6, olen=n % 4 == 2)
  _add("fwd", 233, 8, 2, 37, variant=0)
  # ---- weight gradient
  for i, K in enumerate(MF_K):
    _add("wgrad", K, Cs4[i % 4], (2, 3, 4)[i % 3], (927, 928, 929)[(i + i // 3) % 3], pad="valid" if i % 4 == 3 else "same",
         ragged=i % 5 != 4)
  _add("wgrad", 33, 24, 2, 1900)
  wwin = [(1, 1), (97, 1), (129, 1), (256, 1), (39, 2), (87, 2), (20, 4), (64, 4), (33, 1), (39, 2), (20, 4)]
  for i, (K, d) in enumerate(wwin):
    _add("wgrad", K, Cs5[i % 5], (3, 2, 4)[i % 3], (255, 256, 257, 299)[(i + i // 4) % 4], d=d,
         pad="valid" if i % 4 == 2 else "same", variant=1 if K == 33 else -1, ragged=i % 6 != 5)
  wgen = [(65, 1, 4, -1), (129, 1, 2, -1), (257, 1, 1, -1), (7, 1, 3, -1), (11, 2, 1, -1), (2, 1, 1, 0), (33, 1, 1, 0),
          (75, 1, 1, 0), (129, 1, 1, 0)]
  for i, (K, s, d, v) in enumerate(wgen):
    _add("wgrad", K, Cs5[(i + 1) % 5], (2, 3, 4)[i % 3], (127, 128, 129, 261)[i % 4], s=s, d=d,
         pad="valid" if i % 4 == 1 else "same", variant=v, ragged=i % 5 != 3)
  _add("wgrad", 313, 8, 2, 37)
  # ---- fused data gradient: pad names the FORWARD convolution (same: padL = K - 1 - SAME; valid: Tout = Tin + K - 1)
  for i, K in enumerate(FUSED_K):
    Tt = dm_geom(K)["tile"]
    for j in range(2):
      n = 2 * i + j
      _add("fused", K, (8, 40)[(n + n // 2) % 2], (3, 4, 2)[n % 3], (300, Tt, 2 * Tt + 5)[(n + n // 3) % 3],
           pad="valid" if n == 4 else "full" if n == 9 else "same", ragged=n != 7, addend=("none", "sep", "alias")[n % 3],
           scale=(1.0, 0.8)[(n // 3) % 2])


_build()


def geometry(name):
  """Tin, Tout, padL of a case and its dispatch class."""
  s = CASES[name]
  K, T, st, d, pad = s["K"], s["T"], s["s"], s["d"], s["pad"]
  if s["op"] == "fused":
    # data gradient of a stride-1 forward convolution: dz has the forward's output rows, dx its input rows
    if pad == "same":
      tin, padl = T, K - 1 - same_padding(T, K, 1, 1)[1]
    elif pad == "valid":            # forward VALID: dz is K - 1 rows shorter than dx
      tin, padl = T - (K - 1), K - 1
    else:                           # forward FULL: dz is K - 1 rows longer
      tin, padl = T + (K - 1), 0
    return dict(tin=tin, tout=T, padl=padl, cls=fwd_class(K, 1, 1, -1))
  if pad == "same":
    tin = T if st == 1 else T * st - 1
    tout, padl = same_padding(tin, K, st, d)
    assert tout == T
  elif pad == "valid":
    tin, padl = (T - 1) * st + (K - 1) * d + 1, 0
  else:
    tin, padl = (T - 1) * st + 1 - (K - 1) * d, (K - 1) * d
  assert tin >= 1 and padl >= 0, name
  cls = (fwd_class if s["op"] == "fwd" else wgrad_class)(K, st, d, s["variant"])
  return dict(tin=tin, tout=T, padl=padl, cls=cls)


def _lens(B, T):
  """Ragged lengths: a full sample, a 0 and a 1 where the batch has room, and one that ends inside the first of
  several tiles (the later tiles of that sample are dead: their input window lies past the end)."""
  mid = max(2, (2 * T) // 5)
  return {2: [T, mid], 3: [T, 1, mid], 4: [T, 0, 1, mid], 5: [T, 0, 1, mid, T - 1]}[B]


def make_inputs(name):
  s = dict(CASES[name])
  s.update(geometry(name))
  B, C, K, tin, tout = s["B"], s["C"], s["K"], s["tin"], s["tout"]
  g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
  s["w"] = torch.randn(K, C, generator=g) * 0.5
  s["x"] = torch.randn(B, tin, C, generator=g).to(BF16)
  if s["init"] == "split":
    # x = 1, w[k] = sg[k] h[k] + 0.9 * 2^-9 h[k] with h bf16 in [0.51, 1), h[2i + 1] = h[2i], sg = +1, -1, ...: the bf16
    # parts sg h cancel exactly and the result is the sum of the remainders, 0.9 * 2^-9 sum h (below half a bf16 ulp of
    # every w[k]: hi = sg h). A kernel without the lo table gives 0.
    assert K % 2 == 0
    h = (0.51 + 0.48 * torch.rand(K // 2, C, generator=g)).to(BF16).double().repeat_interleave(2, 0)
    sg = torch.tensor([1.0, -1.0], dtype=F64).repeat(K // 2)[:, None]
    s["w"] = (sg * h + 0.9 * 2.0 ** -9 * h).float()
    assert torch.equal(s["w"].to(BF16).double(), sg * h)
    s["x"] = torch.ones(B, tin, C, dtype=BF16)
  s["in_len"] = torch.tensor(_lens(B, tin), dtype=torch.int32) if s["ragged"] else None
  if s["op"] == "fwd":
    s["out_len"] = None
    if s["olen"] and s["ragged"]:
      s["out_len"] = torch.clamp((s["in_len"] + s["s"] - 1) // s["s"], max=tout).to(torch.int32)
  elif s["op"] == "wgrad":
    s["dy"] = torch.randn(B, tout, C, generator=g).to(BF16)
    s["dw0"] = torch.randn(K, C, generator=g)
  else:
    s["in_len"] = None
    s["out_len"] = torch.tensor(_lens(B, tout), dtype=torch.int32) if s["ragged"] else None
    live = live_rows(s["out_len"], B, tout)
    # a ReLU output stored masked: exact zeros in about half of the live elements and in every row t >= out_len
    s["mask_ref"] = torch.where(live, torch.randn(B, tout, C, generator=g).clamp_min(0.0), 0.0).to(BF16)
    s["stat_ref"] = torch.randn(B, tout, C, generator=g).to(BF16)
    s["addend_t"] = None if s["addend"] == "none" else torch.randn(B, tout, C, generator=g).to(BF16)
    s["mask_scale"] = float(f32(1.0) / f32(s["scale"]))       # fp32 quotient, as the caller forms it
  return s


# ---------------------------------------------------------------------------------------------------------
# float64 oracles
# ---------------------------------------------------------------------------------------------------------
def mask_rows(x, lens):
  """x with the rows t >= lens[b] zeroed (x itself without a length vector)."""
  if lens is None:
    return x
  B, T = x.shape[:2]
  return torch.where(live_rows(lens, B, T), x, torch.zeros((), dtype=x.dtype))


def tap_rows(xm, K, stride, dil, padl, tout):
  """k -> [B, tout, C]: row t is xm[b, t stride + k dil - padl] (zero outside [0, Tin))."""
  assert padl >= 0
  tin = xm.shape[1]
  span = (tout - 1) * stride + 1
  right = max(0, span + (K - 1) * dil - padl - tin)
  xp = F.pad(xm, (0, 0, padl, right))
  return lambda k: xp[:, k * dil:k * dil + span:stride]


def oracle_fwd(x, w, in_len, tout, stride, dil, padl, flip):
  """y[b,t,c] = sum_k x[b, t s + k d - padL, c] w[k,c] (flip: w[K-1-k]) and sum_k |x w|, float64."""
  K = w.shape[0]
  rows = tap_rows(mask_rows(x.double(), in_len), K, stride, dil, padl, tout)
  wd = w.double().flip(0) if flip else w.double()
  y = torch.zeros(x.shape[0], tout, x.shape[2], dtype=F64)
  mag = torch.zeros_like(y)
  for k in range(K):
    t = rows(k) * wd[k]
    y += t
    mag += t.abs()
  return y, mag


def oracle_wgrad(x, dy, in_len, stride, dil, padl, K):
  """sum_{b,t} dy[b,t,c] x[b, t s + k d - padL, c], the sum of the terms' magnitudes [K, C] and the number of
  (b, t) terms whose x row exists [K, 1]."""
  B, tout, C = dy.shape
  rows = tap_rows(mask_rows(x.double(), in_len), K, stride, dil, padl, tout)
  ones = tap_rows(mask_rows(torch.ones(B, x.shape[1], 1, dtype=F64), in_len), K, stride, dil, padl, tout)
  d = dy.double()
  S, A, n = torch.zeros(K, C, dtype=F64), torch.zeros(K, C, dtype=F64), torch.zeros(K, 1, dtype=F64)
  for k in range(K):
    t = rows(k) * d
    S[k], A[k], n[k] = t.sum((0, 1)), t.abs().sum((0, 1)), ones(k).sum()
  return S, A, n


def row_tiles(x, n):
  """[B, T, C] -> [B * ceil(T / n), n, C], zero padded: the time tiles of every sample."""
  B, T, C = x.shape
  nt = ceil_div(T, n)
  return F.pad(x, (0, 0, 0, nt * n - T)).reshape(B * nt, n, C)


# ---------------------------------------------------------------------------------------------------------
# compare()
# ---------------------------------------------------------------------------------------------------------
def conv_bound(cls, K, mag):
  """Bound of the fp32 convolution before its bf16 store.
  VALU kernels (generic, register window): K fused multiply-adds per output, each rounding relative to a partial sum
  of at most sum_k |x w|: K u32 sum|x w| (an unfused product and K - 1 additions: the same).
  Matrix cores: the window of an output has 16 Jt positions and every step issues two MFMAs (hi, lo), so the sum has
  32 Jt terms (the products bf16 x bf16 are exact): 32 Jt u32 sum|x (hi + lo)|. The taps enter as hi = bf16(w),
  lo = bf16(w - hi): for w in [2^e, 2^(e+1)) the remainder r = w - hi is exact in fp32 with |r| <= 2^(e-8); |r| =
  2^(e-8) is a power of two, hence lo = r; otherwise |r| < 2^(e-8) and lo rounds it to half a bf16 ulp of a number below
  2^(e-8), 2^(e-9-8) = 2^(e-17) <= 2^-17 |w| (half of that unless r sits in the top binade; the factor 2 covers the ties
  to even there). So |w - hi - lo| <= 2^-17 |w| and the split adds 2^-17 sum|x w|."""
  if cls[0] == "mfma":
    return (32 * cls[1] * U32 + SPLIT_RESIDUAL) * mag
  return K * U32 * mag


def _cmp_fwd(got, inp, chk):
  # |y - ref| <= ubf |ref| + conv_bound: the bf16 store rounds the fp32 sum once (RNE errs by at most
  # ubf / (1 + ubf) of the value it rounds; that margin takes the second-order term ubf * conv_bound)
  y = got["y"]
  B, tout, C = y.shape
  K = inp["w"].shape[0]
  cls = fwd_class(K, inp["stride"], inp["dil"], inp["variant"])
  ref, mag = oracle_fwd(inp["x"], inp["w"], inp["in_len"], tout, inp["stride"], inp["dil"], inp["pad_left"], inp["flip"])
  asserted = live_rows(inp["out_len"], B, tout)
  bound = UBF * ref.abs() + conv_bound(cls, K, mag)
  yv = torch.where(asserted, y, torch.zeros((), dtype=BF16))
  chk.within("y", yv, torch.where(asserted, ref, 0.0), torch.where(asserted, bound, 0.0))


# The rounding inside an MFMA's own accumulation (32 products per v_mfma_f32_16x16x32_bf16) is not documented; an
# integer factor on the two matrix-core weight-gradient bounds would go here. Measured ratio 4.0e-4: it stays 1.
MFMA_WGRAD_FACTOR = 1
_wgrad_memo = []


def _cmp_wgrad(got, inp, chk):
  # dy x is exact in fp32 (bf16 x bf16), so only additions round: a sum of n terms in ANY order - threads, LDS trees,
  # atomics across workgroups - errs by at most (n - 1) u32 sum|terms|, n = the (b, t) terms of the element whose x
  # row exists; n u32 sum|terms| is asserted. dw on entry takes part in the W additions that reach the element (one
  # per contributing workgroup, wgrad_adds), each rounding a partial result of at most |dw0| + sum|terms|:
  # W u32 (|dw0| + sum|terms|) on top when dw0 is not zero.
  dw0, K = inp["dw0"], inp["dw0"].shape[0]
  B, tout, C = inp["dy"].shape
  cls = wgrad_class(K, inp["stride"], inp["dil"], inp["variant"])
  key = (inp["x"], inp["dy"], inp["in_len"], inp["stride"], inp["dil"], inp["pad_left"], K)
  if len(_wgrad_memo) != 2 or any(a is not b for a, b in zip(_wgrad_memo[0], key)):
    _wgrad_memo[:] = [key, oracle_wgrad(*key)]        # the runs of one case share their reference
  S, A, n = _wgrad_memo[1]
  bound = n * U32 * A
  if bool((dw0 != 0).any()):
    bound = bound + wgrad_adds(cls, B, tout, C, inp["det"]) * U32 * (dw0.double().abs() + A)
  chk.within("dw", got["dw"], dw0.double() + S, bound * MFMA_WGRAD_FACTOR if cls[0] == "mfma" else bound)


def _cmp_fused(got, inp, chk):
  # The kernel rounds the convolution to bf16 in the plane, then adds the addend, masks, scales and rounds again:
  #   |dx - ref| <= ubf |ref| + mask_scale (ubf |conv| + conv_bound)
  # (the fp32 addition and product in between, 2 u32 |ref|, sit in the margin ubf^2 |ref| of the RNE bound);
  # exactly +0 where mask_ref <= 0 and in every row t >= out_len.
  dx, stats = got["dx"], got["stats"]
  B, tout, C = dx.shape
  K = inp["w"].shape[0]
  cls = fwd_class(K, 1, 1, -1)
  assert cls[0] == "mfma"
  conv, mag = oracle_fwd(inp["dz"], inp["w"], None, tout, 1, 1, inp["pad_left"], 1)
  scale = float(f32(inp["mask_scale"]))
  passes = inp["mask_ref"].float() > 0
  ad = inp["addend"].double() if inp["addend"] is not None else 0.0
  ref = torch.where(passes, (conv + ad) * scale, 0.0)
  bound = UBF * ref.abs() + scale * (UBF * conv.abs() + conv_bound(cls, K, mag))
  chk.within("dx", dx, ref, torch.where(passes, bound, 0.0))
  chk.bits("dx: +0 where mask_ref <= 0", dx, torch.zeros_like(dx), ~passes)
  chk.bits("dx: +0 at t >= out_len", dx, torch.zeros_like(dx), ~live_rows(inp["out_len"], B, tout).expand(B, tout, C))
  # stats[part, 0 | 1, c] = sum over the tile's rows of the STORED dx | of dx stat_ref, part = b ntt + tile. The kernel
  # (store phase) adds per thread at most ceil(tile / 4 * 4 / 512) = 2 items x 4 rows, then one thread adds the 128
  # thread partials of its 8-channel group in sequence: a depth of 8 + 128 additions, depth u32 sum|terms|, and one
  # rounding per product for stats[:, 1]. A tile past out_len is not visited: exact zeros (all its dx are +0).
  Tt = dm_geom(K)["tile"]
  assert tuple(stats.shape) == (num_parts(B, tout, K), 2, C), stats.shape
  depth = ceil_div(ceil_div(Tt, 4) * 4, 512) * 4 + 128
  D = row_tiles(dx.double(), Tt)
  DS = D * row_tiles(inp["stat_ref"].double(), Tt)
  chk.within("stats[0]", stats[:, 0], D.sum(1), depth * U32 * D.abs().sum(1))
  chk.within("stats[1]", stats[:, 1], DS.sum(1), (depth + 1) * U32 * DS.abs().sum(1))


_STAGES = {"fwd": _cmp_fwd, "wgrad": _cmp_wgrad, "fused": _cmp_fused}
STAGES = tuple(_STAGES)


def compare(stage, got, inp):
  """One operation's outputs `got` against the float64 oracle of its inputs `inp`:
  ({output: largest error / bound}, [a line per output that breaks its bound])."""
  chk = _Checks()
  _STAGES[stage](got, inp, chk)
  return chk.ratios, chk.fails


# ---------------------------------------------------------------------------------------------------------
# the walks
# ---------------------------------------------------------------------------------------------------------
class _Run:
  def __init__(self, name, log):
    self.name, self.log, self.ratios, self.fails = name, log, {}, []

  def cmp(self, stage, got, inp, tag=""):
    ratios, fails = compare(stage, got, inp)
    for k, v in ratios.items():
      key = "%s.%s" % (stage, k.split(":")[0])
      self.ratios[key] = max(self.ratios.get(key, 0.0), v)
    self.fails.extend("%s %s %s" % (self.name, tag, f) for f in fails)

  def same(self, what, a, b, mask=None):
    chk = _Checks()
    chk.bits(what, a, b, mask)
    self.fails.extend("%s %s" % (self.name, f) for f in chk.fails)

  def done(self):
    for k in sorted(self.ratios):
      self.log("DW-RATIO %-52s %-14s %.3g" % (self.name, k, self.ratios[k]))
    for f in self.fails:
      self.log("DW-FAIL " + f)
    return dict(fails=self.fails, ratios=self.ratios)


def poisoned(x, lens, poison):
  if lens is None:
    return x
  B, T = x.shape[:2]
  return torch.where(live_rows(lens, B, T), x, torch.full((), poison, dtype=x.dtype))


def check_case(name, be, log=print, poison=math.nan):
  """Runs case `name` on backend `be`. Returns dict(fails, ratios): fails is empty iff every output kept its bound."""
  R = make_inputs(name)
  run = _Run(name, log)
  st = dict(stride=R["s"], dil=R["d"], pad_left=R["padl"], variant=R["variant"])
  if R["op"] == "fwd":
    args = dict(st, w=R["w"], in_len=R["in_len"], out_len=R["out_len"], tout=R["tout"], flip=R["flip"])
    xp = poisoned(R["x"], R["in_len"], poison)
    y = be.fwd(x=xp, **args)
    assert tuple(y.shape) == (R["B"], R["tout"], R["C"]) and y.dtype == BF16
    run.cmp("fwd", dict(y=y), dict(args, x=xp))
    if R["in_len"] is not None:
      y2 = be.fwd(x=mask_rows(R["x"], R["in_len"]), **args)
      run.same("fwd: y unchanged by the rows t >= in_len", y, y2, live_rows(R["out_len"], R["B"], R["tout"]))
  elif R["op"] == "wgrad":
    args = dict(st, dy=R["dy"], in_len=R["in_len"])
    xp = poisoned(R["x"], R["in_len"], poison)
    zero = torch.zeros_like(R["dw0"])
    for dw0, det, tag in ((zero, False, "dw = 0"), (R["dw0"], False, "dw != 0"), (zero, True, "det dw = 0"),
                          (R["dw0"], True, "det dw != 0")):
      dw = be.wgrad(x=xp, dw0=dw0, det=det, **args)
      run.cmp("wgrad", dict(dw=dw), dict(args, x=xp, dw0=dw0, det=det), tag)
    again = be.wgrad(x=xp, dw0=R["dw0"], det=True, **args)
    run.same("wgrad: deterministic mode, two runs", dw, again)
    if R["in_len"] is not None:
      clean = be.wgrad(x=mask_rows(R["x"], R["in_len"]), dw0=R["dw0"], det=True, **args)
      run.same("wgrad: dw unchanged by the rows t >= in_len (deterministic mode)", dw, clean)
  else:
    assert be.num_parts(R["B"], R["tout"], R["K"]) == num_parts(R["B"], R["tout"], R["K"])
    args = dict(dz=R["x"], w=R["w"], addend=R["addend_t"], mask_ref=R["mask_ref"], stat_ref=R["stat_ref"],
                out_len=R["out_len"], pad_left=R["padl"], mask_scale=R["mask_scale"])
    dx, stats = be.fused(alias=R["addend"] == "alias", **args)
    run.cmp("fused", dict(dx=dx, stats=stats), args)
  return run.done()
