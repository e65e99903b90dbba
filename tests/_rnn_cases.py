"""Helper of tests/test_rnn_paths_gpu.py and tests/test_rnn_oracle_cpu.py (not a test module): the case
table that reaches every dispatch class of os2s_rnn_layer_fwd_multi / os2s_rnn_layer_bwd_multi, a float64
oracle of the recurrence alone (it takes gx, not x: the GEMM side stays with tests/test_rnn_gpu.py), the
device run and the comparison of the two.

Oracle. forward_oracle() is the three cells of csrc/rnn.hip:3-12 / include/os2s.h in float64: R plainly,
R_b with a straight-through bf16 round where the kernels store bf16 (the h fed to the next step's product,
y, the saved gates; the direct z * h path and c stay unrounded, as h32 / hst / c32 do). backward_oracle() is
teacher-forced on the tensors the kernel itself saved (gates, c_seq, y as read back from the device) plus
dy and wh, so the forward's rounding stays out of the backward bound; R_b rounds the gate gradients handed
from step s + 1 to step s (dg_cur), the stored dgx / dgr and, for the persistent backward, each producer's
partial dh block before the 32-term sum (rnn_xcd.hip, phase 3; a producer's units are upc = ceil(H / 32)
consecutive ones).

compare(): every output elementwise, live rows chosen with torch.where,
    |got - R_b| <= 4 n_q + 2^-7 |R_b|
n_q = max over the cases of a cell of max|R_b.q - R.q| (noise_floor(): oracle alone, on the CPU; for the
backward outputs the teacher is the forward R_b). One more rounding per store than R_b has doubles n_q, a
flipped rounding doubles it again; the floor is one bf16 ulp of the element, the last store. Exact: y, dgx,
dgr rows at or past a sample's length are zero (a length of 0: the whole sample); a length above T behaves
as T (the oracle clamps as the kernels do, and a rerun with the lengths clamped on the host gives the same
bits); the guard columns of the strided runs keep their sentinel and a contiguous rerun gives the same bits;
a second launch of a persistent case gives the same bits on live rows. The two directions of an ndir = 2
launch have their own gx, wh, bh, dy and their own single-direction oracle.

Kernel instances per case, read off the host predicates (rnn.hip: rows8 = ceil(H/32) ceil(B/32) ndir < 128;
rnn_xcd.hip: gru_xcd_supported / gru_xcd_bwd_supported, RT = 5 for 3 ceil(H/32) <= 80). fwd<G> =
rnn_step_fwd_kernel<G>, bwd<G,R> = rnn_step_bwd_kernel<G,R>, xcd<NB,RT> = gru_xcd_fwd_kernel<NB,RT>,
xcd bwd = gru_xcd_bwd_kernel; G = 3 for the GRU, 4 for both LSTMs:
  h8             fwd<G>, bwd<G,8>; H = 8: the K - 8 clamp of tile_gemm_prefetch is 0, the upper half-wave is
                 padding; lengths 0 and T + 3 (the clamps); one forward and one reversed launch
  t1             fwd<G>, bwd<G,8>; T = 1 (only the `first` backward step; the GRU is below the persistent
                 path's T >= 2 and H >= 32), K = 24 and G K = 72: K % 16 == 8
  b33_h24        fwd<G>, bwd<G,8>; second batch tile holding one sample; strided y / dy
  h1032          fwd<G> two rounds (K = 1032 > 8 waves x 8 x 16); bwd<3,8> two rounds (3096 > 2432),
                 bwd<4,8> three rounds (4128 > 2 x 2048)
  rows32_h72     fwd<G>, bwd<G,32> (3 x 22 x 2 = 132 >= 128) with H % 32 = 8: the j0 + l31 < H row guard
  x_h40          xcd<1,5> + xcd bwd; upc = 2: workgroups 20..31 own no unit, NK = 2 with a partial k-step
  x_h808         xcd<1,5> + xcd bwd; upc = 26: the last workgroup owns 2 units
  x_h840         xcd<1,6> + xcd bwd above H = 800; upc = 27: the last workgroup owns 3 units; reversed only
  x_h1024        xcd<1,6> at its top (upc = 32); bwd<3,8> two rounds (H > 896 = 8 kXcdBT 16)
  x_b17_h840     xcd<2,6>, 163 466 B of dynamic LDS against 163 584; bwd<3,8> (B > 16)
  x_b32_h104_t2  xcd<2,5>, T = 2, upc = 4: workgroups 26..31 own no unit; bwd<3,8>; strided y / dy

Measured. n_q (float64 oracle, all cases of the cell; the tests compute their own at run time):
  gru          y 2.187e-3  gates 4.280e-3  dgx 8.236e-3  dgr 4.405e-3
  lstm_cudnn   y 1.633e-3  gates 2.520e-3  c_seq 5.628e-4  dgx 4.019e-3
  lstm_tf      y 1.098e-3  gates 2.286e-3  c_seq 7.128e-4  dgx 3.571e-3
Largest err / bound on the MI355X, per case and output over its directions (0: bit-identical to R_b). No
rounding had to be added to R_b: the persistent kernels' tanh_fast_ / __expf stay inside the bound.
  h8-gru                 y 0        gates 0        dgx 0        dgr 0
  h8-lstm_cudnn          y 0        gates 0        c_seq 2.0e-5 dgx 0
  h8-lstm_tf             y 0        gates 0        c_seq 2.0e-5 dgx 0
  t1-gru                 y 0        gates 0        dgx 0        dgr 0
  t1-lstm_cudnn          y 0        gates 0        c_seq 9.4e-6 dgx 0
  t1-lstm_tf             y 0        gates 0        c_seq 8.0e-6 dgx 0
  b33_h24-gru            y 3.4e-6   gates 0        dgx 0        dgr 0
  b33_h24-lstm_cudnn     y 0        gates 0        c_seq 2.7e-5 dgx 0
  b33_h24-lstm_tf        y 0        gates 0        c_seq 2.5e-5 dgx 8.4e-3
  h1032-gru              y 0        gates 1.7e-6   dgx 0        dgr 0
  h1032-lstm_tf          y 0        gates 0        c_seq 3.1e-5 dgx 1.3e-4
  rows32_h72-gru         y 1.7e-1   gates 1.0e-1   dgx 1.0e-1   dgr 9.2e-2
  rows32_h72-lstm_cudnn  y 1.3e-1   gates 2.7e-1   c_seq 4.9e-2 dgx 1.0e-1
  x_h40-gru              y 0        gates 0        dgx 0        dgr 0
  x_h808-gru             y 1.8e-1   gates 1.9e-1   dgx 5.5e-2   dgr 2.7e-2
  x_h840-gru             y 9.7e-2   gates 2.7e-2   dgx 5.6e-2   dgr 0
  x_h1024-gru            y 1.8e-1   gates 1.8e-1   dgx 1.5e-2   dgr 2.7e-5
  x_b17_h840-gru         y 5.2e-2   gates 9.8e-2   dgx 5.3e-2   dgr 1.7e-3
  x_b32_h104_t2-gru      y 0        gates 1.8e-1   dgx 9.3e-4   dgr 5.4e-5"""
import functools
import math
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
  sys.path.insert(0, REPO)

GRU, LSTM_CUDNN, LSTM_TF = "gru", "lstm_cudnn", "lstm_tf"
CELL_ID = {GRU: 0, LSTM_CUDNN: 1, LSTM_TF: 2}
ALL3 = (GRU, LSTM_CUDNN, LSTM_TF)
RAGGED = "ragged"

# name: cells, launches (tuples of reverse flags: one tuple = one launch), B, T, H, lens, strided,
#       GRU forward path, GRU backward path ("step" / "xcd"; the LSTMs always take the step kernels)
CASES = {
    "h8": (ALL3, ((0,), (1,)), 5, 7, 8, [7, 1, 4, 0, 10], False, "step", "step"),
    "t1": (ALL3, ((0, 1),), 3, 1, 24, None, False, "step", "step"),
    "b33_h24": (ALL3, ((0, 1),), 33, 4, 24, RAGGED, True, "step", "step"),
    "h1032": ((GRU, LSTM_TF), ((0,),), 3, 3, 1032, RAGGED, False, "step", "step"),
    "rows32_h72": ((GRU, LSTM_CUDNN), ((0, 1),), 675, 3, 72, RAGGED, False, "step", "step"),
    "x_h40": ((GRU,), ((0, 1),), 3, 5, 40, RAGGED, False, "xcd", "xcd"),
    "x_h808": ((GRU,), ((0, 1),), 16, 4, 808, RAGGED, False, "xcd", "xcd"),
    "x_h840": ((GRU,), ((1,),), 9, 3, 840, RAGGED, False, "xcd", "xcd"),
    "x_h1024": ((GRU,), ((0, 1),), 16, 3, 1024, None, False, "xcd", "step"),
    "x_b17_h840": ((GRU,), ((0, 1),), 17, 3, 840, RAGGED, False, "xcd", "step"),
    "x_b32_h104_t2": ((GRU,), ((0, 1),), 32, 2, 104, None, True, "xcd", "step"),
}
RUNS = [(n, c) for n in CASES for c in CASES[n][0]]
SEED = {}                 # (case, cell) -> seed override; default: sum of the code points of "case-cell"
FORGET_BIAS = 1.0
SENTINEL = -7.0           # fill of the wider [B, T, 8 + 2H + 8] tensors of the strided runs
GUARD = 8


def outputs_of(cell):
  """y, gates, dgx always; c_seq for the LSTMs; dgr for the GRU (the LSTMs' dgr is their dgx)."""
  return ("y", "gates", "dgx", "dgr") if cell == GRU else ("y", "gates", "c_seq", "dgx")


def spec(case):
  cells, launches, B, T, H, lens, strided, fpath, bpath = CASES[case]
  return dict(cells=cells, launches=launches, B=B, T=T, H=H, lens=lens, strided=strided, fwd=fpath, bwd=bpath,
              dirs=tuple(r for l in launches for r in l))


def paths(case, cell):
  """("step" | "xcd") of the forward and of the backward launch."""
  s = spec(case)
  return (s["fwd"], s["bwd"]) if cell == GRU else ("step", "step")


def rb(x):
  """bf16 round of a float64 tensor (round to nearest even, as f2bf)."""
  return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _id(x):
  return x


@functools.lru_cache(maxsize=None)
def build_inputs(case, cell):
  """bf16-rounded inputs of one (case, cell) from a seeded CPU generator: dict(lens int32 [B] | None,
  dirs = [dict(reverse, gx, wh, bh, dy)] in launch order). CPU tensors; callers must not modify them."""
  s = spec(case)
  B, T, H = s["B"], s["T"], s["H"]
  G = 3 if cell == GRU else 4
  g = torch.Generator().manual_seed(SEED.get((case, cell), sum(map(ord, case + "-" + cell))))
  rn = lambda *sh, sc=1.0: (torch.randn(*sh, generator=g) * sc).to(torch.bfloat16)
  lens = s["lens"]
  if lens == RAGGED:
    lens = torch.randint(1, T + 1, (B,), generator=g, dtype=torch.int32)
    lens[0], lens[1] = T, 1
  elif lens is not None:
    lens = torch.tensor(lens, dtype=torch.int32)
  if lens is not None:
    assert 1 in lens.tolist() and T in lens.tolist()
  dirs = []
  for rev in s["dirs"]:
    dirs.append(dict(reverse=bool(rev), gx=rn(B, T, G * H, sc=0.5), wh=rn(G * H, H, sc=1.0 / math.sqrt(H)),
                     bh=rn(G * H, sc=0.1).float(), dy=rn(B, T, H)))
  return dict(lens=lens, dirs=dirs)


def eff_lens(lens, B, T):
  """min(max(len, 0), T), as all four kernels clamp; T everywhere without lengths."""
  return torch.full((B,), T, dtype=torch.int64) if lens is None else lens.to(torch.int64).clamp(0, T)


def live_steps(case, cell):
  s = spec(case)
  ln = eff_lens(build_inputs(case, cell)["lens"], s["B"], s["T"])
  return torch.arange(s["T"])[None, :] < ln[:, None]


def _sig(x):
  return 1.0 / (1.0 + torch.exp(-x))


# mutations of the oracle (tests/test_rnn_oracle_cpu.py): a deliberately wrong recurrence compare() must reject
FWD_MUTATIONS = ("tf_gates_in_cudnn_order", "no_forget_bias", "gru_bias_outside_r", "reverse_from_T")
BWD_MUTATIONS = ("dgr_is_dgx", "no_dhz_carry_unit", "no_dc_carry_step")


def forward_oracle(cell, gx, wh, bh, lens, reverse, forget_bias=FORGET_BIAS, rounded=False, mutate=None):
  """The recurrence in float64. gx [B,T,G*H], wh [G*H,H], bh [G*H] | None, lens [B] | None. Returns y [B,T,H],
  gates [B,T,4H] in the layout the kernels save (GRU: r, z, n, R_n h + b_Rn; both LSTMs: i, f, g, o as
  activations) and c_seq [B,T,H] (LSTMs). Rows of finished steps are zero."""
  gx, wh = gx.double(), wh.double()
  B, T, GH = gx.shape
  H = wh.shape[1]
  G = GH // H
  assert G == (3 if cell == GRU else 4)
  bias = torch.zeros(GH, dtype=torch.float64) if bh is None else bh.double()
  ln = eff_lens(lens, B, T)
  rd = rb if rounded else _id
  order = cell
  if mutate == "tf_gates_in_cudnn_order":
    assert cell == LSTM_TF
    order = LSTM_CUDNN
  fb = forget_bias if (cell == LSTM_TF and mutate != "no_forget_bias") else 0.0
  h = torch.zeros(B, H, dtype=torch.float64)
  c = torch.zeros(B, H, dtype=torch.float64)
  hb = torch.zeros(B, H, dtype=torch.float64)
  y = torch.zeros(B, T, H, dtype=torch.float64)
  gates = torch.zeros(B, T, 4 * H, dtype=torch.float64)
  c_seq = torch.zeros(B, T, H, dtype=torch.float64)
  bi = torch.arange(B)
  for s in range(T):
    act = (s < ln)[:, None]
    first = torch.full_like(ln, T - 1) if mutate == "reverse_from_T" else ln - 1
    t = ((first - s) if reverse else torch.full_like(ln, s)).clamp(0, T - 1)
    pre = gx[bi, t].view(B, G, H)
    rec = (hb @ wh.t() + bias).view(B, G, H)
    if cell == GRU:
      r = _sig(pre[:, 0] + rec[:, 0])
      z = _sig(pre[:, 1] + rec[:, 1])
      hn = rec[:, 2]
      if mutate == "gru_bias_outside_r":
        n = torch.tanh(pre[:, 2] + r * (hn - bias[2 * H:]) + bias[2 * H:])
      else:
        n = torch.tanh(pre[:, 2] + r * hn)
      hnew = (1.0 - z) * n + z * h
      cnew = c
      sv = torch.cat([r, z, n, hn], dim=1)
    else:
      a = pre + rec
      if order == LSTM_CUDNN:
        ig, fg, gg, og = _sig(a[:, 0]), _sig(a[:, 1] + fb), torch.tanh(a[:, 2]), _sig(a[:, 3])
      else:
        ig, gg, fg, og = _sig(a[:, 0]), torch.tanh(a[:, 1]), _sig(a[:, 2] + fb), _sig(a[:, 3])
      cnew = c * fg + ig * gg
      hnew = torch.tanh(cnew) * og
      sv = torch.cat([ig, fg, gg, og], dim=1)
    h = torch.where(act, hnew, h)        # past the end the state passes through
    c = torch.where(act, cnew, c)
    hb = rd(h)
    y[bi, t] = torch.where(act, rd(hnew), y[bi, t])
    gates[bi, t] = torch.where(act, rd(sv), gates[bi, t])
    c_seq[bi, t] = torch.where(act, cnew, c_seq[bi, t])
  out = dict(y=y, gates=gates)
  if cell != GRU:
    out["c_seq"] = c_seq
  return out


def backward_oracle(cell, gates, c_seq, y, dy, wh, lens, reverse, rounded=False, xcd=False, mutate=None,
                    mutate_at=0):
  """Backward through time in float64, teacher-forced on the saved gates / c_seq / y. Returns dgx and dgr
  [B,T,G*H] (gate order of gx: GRU r, z, n; cuDNN LSTM i, f, g, o; LSTMCell i, j, f, o), zero on finished
  steps. xcd (with rounded): each producer's partial dh block is rounded before the 32-term sum.
  mutate_at: the unit (no_dhz_carry_unit) or loop step (no_dc_carry_step) a mutation hits."""
  gates, y, dy, wh = gates.double(), y.double(), dy.double(), wh.double()
  B, T, H = dy.shape
  GH = wh.shape[0]
  G = GH // H
  ln = eff_lens(lens, B, T)
  rd = rb if rounded else _id
  dgx = torch.zeros(B, T, GH, dtype=torch.float64)
  dgr = torch.zeros(B, T, GH, dtype=torch.float64)
  dg_next = torch.zeros(B, GH, dtype=torch.float64)
  carry = torch.zeros(B, H, dtype=torch.float64)
  dcarry = torch.zeros(B, H, dtype=torch.float64)
  bi = torch.arange(B)
  zero = torch.zeros((), dtype=torch.float64)
  if rounded and xcd:
    upc = (H + 31) // 32
    whp = torch.zeros(G, 32 * upc, H, dtype=torch.float64)
    whp[:, :H] = wh.view(G, H, H)
    whp = whp.view(G, 32, upc, H)
  for s in range(T - 1, -1, -1):
    act = (s < ln)[:, None]
    t = ((ln - 1 - s) if reverse else torch.full_like(ln, s)).clamp(0, T - 1)
    tp = (t + 1 if reverse else t - 1).clamp(0, T - 1)
    if rounded and xcd:
      dgp = torch.zeros(B, G, 32 * upc, dtype=torch.float64)
      dgp[:, :, :H] = dg_next.view(B, G, H)
      part = torch.einsum("bgcu,gcuj->bcj", dgp.view(B, G, 32, upc), whp)
      rec = rb(part).sum(1)
    else:
      rec = dg_next @ wh
    dh = dy[bi, t] + rec + carry
    sv = gates[bi, t].view(B, 4, H)
    if cell == GRU:
      hprev = y[bi, tp] if s > 0 else torch.zeros(B, H, dtype=torch.float64)
      rg, zg, ng, hn = sv[:, 0], sv[:, 1], sv[:, 2], sv[:, 3]
      dn = dh * (1.0 - zg)
      dz = dh * (hprev - ng)
      dnpre = dn * (1.0 - ng * ng)
      dr = dnpre * hn
      dpre = torch.stack([dr * rg * (1.0 - rg), dz * zg * (1.0 - zg), dnpre], dim=1)
      drec = dpre.clone()
      if mutate != "dgr_is_dgx":
        drec[:, 2] = dnpre * rg
      ncarry = dh * zg
      if mutate == "no_dhz_carry_unit":
        ncarry[:, mutate_at] = 0.0
      ndc = dcarry
    else:
      ig, fg, gg, og = sv[:, 0], sv[:, 1], sv[:, 2], sv[:, 3]
      cv = c_seq.double()[bi, t]
      cprev = c_seq.double()[bi, tp] if s > 0 else torch.zeros(B, H, dtype=torch.float64)
      tc = torch.tanh(cv)
      dox = dh * tc * og * (1.0 - og)
      dc = dh * og * (1.0 - tc * tc) + dcarry
      dix = dc * gg * ig * (1.0 - ig)
      dfx = dc * cprev * fg * (1.0 - fg)
      dgg = dc * ig * (1.0 - gg * gg)
      ndc = dc * fg
      if mutate == "no_dc_carry_step" and s == mutate_at:
        ndc = torch.zeros_like(ndc)
      dpre = torch.stack([dix, dfx, dgg, dox] if cell == LSTM_CUDNN else [dix, dgg, dfx, dox], dim=1)
      drec = dpre
      ncarry = torch.zeros_like(dh)
    dpre, drec = dpre.reshape(B, GH), drec.reshape(B, GH)
    carry = torch.where(act, ncarry, carry)          # a finished sample leaves the carries alone
    dcarry = torch.where(act, ndc, dcarry)
    dg_next = torch.where(act, rd(drec), zero)
    dgx[bi, t] = torch.where(act, rd(dpre), dgx[bi, t])
    dgr[bi, t] = torch.where(act, rd(drec), dgr[bi, t])
  return dict(dgx=dgx, dgr=dgr)


_FWD_CACHE = {}


def reference_fwd(case, cell, rounded):
  """Forward oracle of every direction of a (case, cell): list of dict(y, gates[, c_seq]). Computed once;
  callers must not modify the result."""
  key = (case, cell, rounded)
  if key not in _FWD_CACHE:
    d = build_inputs(case, cell)
    _FWD_CACHE[key] = [forward_oracle(cell, x["gx"], x["wh"], x["bh"], d["lens"], x["reverse"], rounded=rounded)
                       for x in d["dirs"]]
  return _FWD_CACHE[key]


def reference_bwd(case, cell, saved, rounded):
  """Backward oracle of every direction, teacher-forced on `saved` (list of dict(y, gates[, c_seq]))."""
  d = build_inputs(case, cell)
  xcd = paths(case, cell)[1] == "xcd"
  return [backward_oracle(cell, sv["gates"], sv.get("c_seq"), sv["y"], x["dy"], x["wh"], d["lens"], x["reverse"],
                          rounded=rounded, xcd=xcd)
          for x, sv in zip(d["dirs"], saved)]


def _live(t, live):
  """Rows of live steps of a [B, T, C] tensor, zeros elsewhere (never a product with the mask: rows the
  kernels do not write may hold anything)."""
  return torch.where(live[:, :, None], t.double(), torch.zeros((), dtype=torch.float64))


@functools.lru_cache(maxsize=None)
def noise_floor():
  """n_q[cell][q] = max over the cases of the cell and their directions of max|R_b.q - R.q| on live rows: what
  the bf16 stores of the recurrence cost. Oracle alone; the backward is teacher-forced on the forward R_b."""
  n = {c: {q: 0.0 for q in outputs_of(c)} for c in ALL3}
  for case, cell in RUNS:
    live = live_steps(case, cell)
    R, Rb = reference_fwd(case, cell, False), reference_fwd(case, cell, True)
    G, Gb = reference_bwd(case, cell, Rb, False), reference_bwd(case, cell, Rb, True)
    for d in range(len(R)):
      a, b = dict(R[d], **G[d]), dict(Rb[d], **Gb[d])
      for q in outputs_of(cell):
        n[cell][q] = max(n[cell][q], float((_live(b[q], live) - _live(a[q], live)).abs().max()))
  return n


def check_inputs(case, cell):
  """Conditions without which a comparison proves nothing; returns the violations."""
  s = spec(case)
  d = build_inputs(case, cell)
  bad = []
  if d["lens"] is not None:
    l = d["lens"].tolist()
    if min(l) < 0 or max(l) > s["T"] + 3:
      bad.append("%s-%s: a length outside [0, T + 3]" % (case, cell))
    if 1 not in l or s["T"] not in l:
      bad.append("%s-%s: lengths without 1 or T" % (case, cell))
  live = live_steps(case, cell)
  H = s["H"]
  for i, R in enumerate(reference_fwd(case, cell, False)):
    g = _live(R["gates"], live)[live]                            # [rows, 4H]
    sat = (g[:, :2 * H] - 0.5).abs().mul(2.0).mean()             # |2 s - 1| of the first two sigmoid gates
    if not float(sat) < 0.99:
      bad.append("%s-%s dir %d: gates saturated (%.4f)" % (case, cell, i, float(sat)))
  return bad


# ------------------------------------------------------------------------------------------ device
def run_gpu(case, cell, device, strided=None, clamp_lens=False):
  """Forward and backward of one (case, cell) through capi.rnn_layer_{fwd,bwd}_multi, launch by launch, at the
  library's current persistent-kernel mode. Returns dict(dirs = list over directions of CPU tensors dict(y,
  gates[, c_seq], dgx, dgr), wide = per launch of a strided run dict(wide_y, wide_dy)). strided (default: the
  case's own setting): y of both directions are the halves of one [B, T, 8 + 2H + 8] tensor filled with
  SENTINEL, dy is read from slices of another. clamp_lens: the lengths are clamped to [0, T] on the host."""
  from openseq2seq_amd import capi
  s = spec(case)
  B, T, H = s["B"], s["T"], s["H"]
  d = build_inputs(case, cell)
  strided = s["strided"] if strided is None else strided
  lens = None if d["lens"] is None else (d["lens"].clamp(0, T) if clamp_lens else d["lens"]).to(device)
  cid = CELL_ID[cell]
  out, wides = [], []
  k = 0
  for launch in s["launches"]:
    xs = d["dirs"][k:k + len(launch)]
    k += len(launch)
    dev = [{n: (v.to(device) if torch.is_tensor(v) else v) for n, v in x.items()} for x in xs]
    ys = [None] * len(xs)
    dys = [x["dy"] for x in dev]
    if strided:
      assert len(xs) == 2
      wy = torch.full((B, T, GUARD + 2 * H + GUARD), SENTINEL, dtype=torch.bfloat16, device=device)
      wdy = torch.full_like(wy, SENTINEL)
      ys = [wy[:, :, GUARD + i * H:GUARD + (i + 1) * H] for i in range(2)]
      dys = [wdy[:, :, GUARD + i * H:GUARD + (i + 1) * H] for i in range(2)]
      for i in range(2):
        dys[i].copy_(dev[i]["dy"])
    fw = capi.rnn_layer_fwd_multi(cid, [dict(gx=x["gx"], wh=x["wh"], bh=x["bh"], y=ys[i], reverse=x["reverse"])
                                        for i, x in enumerate(dev)], lens, H, forget_bias=FORGET_BIAS)
    torch.cuda.synchronize()
    bw = capi.rnn_layer_bwd_multi(cid, [dict(whT=x["wh"].t().contiguous(), dy=dys[i], y=fw[i][0], gates=fw[i][1],
                                             c_seq=fw[i][2], reverse=x["reverse"]) for i, x in enumerate(dev)],
                                  lens, H, forget_bias=FORGET_BIAS)
    torch.cuda.synchronize()
    for i in range(len(xs)):
      r = dict(y=fw[i][0].cpu().contiguous(), gates=fw[i][1].cpu(), dgx=bw[i][0].cpu(), dgr=bw[i][1].cpu())
      if cell != GRU:
        r["c_seq"] = fw[i][2].cpu()
      out.append(r)
    if strided:
      wides.append(dict(wide_y=wy.cpu(), wide_dy=wdy.cpu()))
  return dict(dirs=out, wide=wides)


def _bits(t):
  return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def same_bits(a, b):
  return a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def compare(case, cell, got, Rb, nq, log=print):
  """The assertions on one result `got` (list over directions of dict(y, gates[, c_seq], dgx, dgr)) against
  R_b (same layout, forward and backward merged); returns the failures (empty: pass) and logs max err / bound
  per output."""
  s = spec(case)
  live = live_steps(case, cell)
  dead = ~live
  ln = eff_lens(build_inputs(case, cell)["lens"], s["B"], s["T"])
  fails = []

  def check(ok, what, *figs):
    log("  %-4s %s-%s %s %s" % ("ok" if ok else "FAIL", case, cell, what, " ".join("%.3e" % f for f in figs)))
    if not ok:
      fails.append("%s-%s: %s %s" % (case, cell, what, " ".join("%.3e" % f for f in figs)))

  for d, (g, r) in enumerate(zip(got, Rb)):
    for q in ("y", "dgx", "dgr"):
      if bool(dead.any()):
        check(bool((g[q].double()[dead] == 0.0).all()), "dir %d %s rows of finished steps exactly zero" % (d, q))
    for b in (ln == 0).nonzero().flatten().tolist():
      check(all(bool((g[q][b].double() == 0.0).all()) for q in ("y", "dgx", "dgr")),
            "dir %d sample %d of length 0 all zero" % (d, b))
    for q in outputs_of(cell):
      a, ref = _live(g[q], live), _live(r[q], live)
      err = (a - ref).abs()
      bound = 4.0 * nq[cell][q] + 2.0 ** -7 * ref.abs()
      ok = bool((err <= bound).all())                # a NaN fails
      worst = float(torch.nan_to_num(err / bound, nan=float("inf")).max())
      check(ok, "dir %d %s vs R_b, 4 n_q + 2^-7 |R_b| (n_q %.3e): max err, max err/bound" % (d, q, nq[cell][q]),
            float(torch.nan_to_num(err, nan=float("inf")).max()), worst)
  return fails


def check_case(case, cell, device, log=print):
  """Device run(s) of one (case, cell) and every assertion on them. Returns (fails, skip_reason): skip_reason is
  set when a persistent case did not reach the persistent kernels (a device without 8 x 32 compute units)."""
  from openseq2seq_amd import capi
  s = spec(case)
  fpath, bpath = paths(case, cell)
  persistent = fpath == "xcd"
  fails = list(check_inputs(case, cell))
  nlaunch = len(s["launches"])
  expect = nlaunch * (int(fpath == "xcd") + int(bpath == "xcd"))
  again = plain = clamped = None
  lens = build_inputs(case, cell)["lens"]
  if cell == GRU and not persistent:
    capi.gru_xcd_set_mode(0)
  try:
    before = capi.gru_xcd_launch_count()
    got = run_gpu(case, cell, device)
    rose = capi.gru_xcd_launch_count() - before
    if persistent and rose == expect:
      again = run_gpu(case, cell, device)
    if s["strided"]:
      plain = run_gpu(case, cell, device, strided=False)
    if lens is not None and (int(lens.min()) < 0 or int(lens.max()) > s["T"]):
      clamped = run_gpu(case, cell, device, clamp_lens=True)
  finally:
    capi.gru_xcd_set_mode(-1)
  log("  %s-%s persistent launches: %d (expected %d)" % (case, cell, rose, expect))
  if persistent and rose == 0:
    return fails, "%s: the persistent GRU kernels were not selected on this device (they need 256 compute units)" % case
  if rose != expect:
    fails.append("%s-%s: %d persistent launches, expected %d" % (case, cell, rose, expect))
  if persistent:
    st = capi.gru_xcd_status(False)
    if st != 0:
      fails.append("%s-%s: os2s_gru_xcd_status = %d after the launches" % (case, cell, st))
  Rb = reference_fwd(case, cell, True)
  Gb = reference_bwd(case, cell, got["dirs"], True)
  fails += compare(case, cell, got["dirs"], [dict(f, **g) for f, g in zip(Rb, Gb)], noise_floor(), log=log)
  H = s["H"]
  for w in got["wide"]:
    for k in ("wide_y", "wide_dy"):
      guard = torch.cat([w[k][:, :, :GUARD], w[k][:, :, GUARD + 2 * H:]], dim=2)
      if not same_bits(guard, torch.full_like(guard, SENTINEL)):
        fails.append("%s-%s: guard columns of %s changed" % (case, cell, k))
  live = live_steps(case, cell)[:, :, None]
  for other, what in ((again, "a second launch"), (plain, "the contiguous run"), (clamped, "host-clamped lengths")):
    if other is None:
      continue
    for d, (a, b) in enumerate(zip(got["dirs"], other["dirs"])):
      for q in outputs_of(cell):
        z = torch.zeros((), dtype=a[q].dtype)
        ok = same_bits(torch.where(live, a[q], z), torch.where(live, b[q], z))
        log("  %-4s %s-%s dir %d %s bit-identical to %s on live rows" % ("ok" if ok else "FAIL", case, cell, d, q, what))
        if not ok:
          fails.append("%s-%s: dir %d %s differs from %s" % (case, cell, d, q, what))
  return fails, None
