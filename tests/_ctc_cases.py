"""Helper of tests/test_ctc_paths_gpu.py and tests/test_ctc_oracle_cpu.py (not a test module): the case table
that reaches every alpha / beta dispatch class of csrc/ctc_loss.hip, a float64 oracle per STAGE, the rounding
bounds, check_case() and the CPU backend (a torch emulation of the kernels' algorithm).

Teacher forcing. Every stage is checked on the tensors the backend itself produced for the previous stage (the
workspace views of capi.ctc_loss(want_workspace=True)); the oracle evaluates the same formula in float64 on
exactly those tensors, so no bound absorbs an upstream stage's rounding. Each bound follows from
    u32 = 2^-24                    unit roundoff of fp32
    exp2 / log2, __expf / __logf   2 ulp (the ISA manual: 1 ulp with denormals flushed; the factor 2 is margin)
and stands next to its code below (_cmp_*); none was fitted to a device run. The end-to-end comparison with
oracle.ctc.ctc_loss_torch (float64) is the seat belt for what teacher forcing cannot see (a wrong initial
condition that the step-0 check shares, a wrong layout).

A backend gives run(inp) -> dict of CPU tensors
    logp [B,T,V] f32, alpha / beta [B,T,Sld] f32 (each row minus its running normaliser), coff_a / coff_b [B,T]
    f64 (the normalisers), loglik [B] f64, valid [B] i32, loss_per_sample [B], loss_mean [1],
    dlogits [T,B,V] f32 or None, dlogits_bf16 [B,T,vpad] bf16 or None
for inp = make_inputs(case, variant). The device backend (test_ctc_paths_gpu.py) prefills the workspace and the
outputs with 0xFF bytes (NaN as float and double), so a dropped store shows. Logits at t >= in_len are NaN, the
label slots past label_len repeat the last label (a valid class id that would add a repeat if it were read), and
one rerun with zeros in place of the NaNs must give the same bits.

Classes reached (os2s_ctc_loss_kernel_class names them; every case asserts its own before it runs):
  ctc_alpha_beta_wave_kernel<4>    w4_edges (T_b = 1, 8 / 9, 32 / 33, L = 0, L + repeats = T_b and T_b + 1),
                                   w4_full (S = 255), w4_repeat (skips allowed and forbidden at lane edges)
  ctc_alpha_beta_wave_kernel<8>    w8_lo (Lmax 128), w8_hi (Lmax 255, V = 32, T_b = 512), w8_repeat, v5_peaky20
  ctc_alpha_beta_wave_kernel<16>   w16_lo (Lmax 256), w16_hi (Lmax 511, S = 1023), w16_repeat
  ctc_alpha_beta_kernel            by V > 32 (t256_v33, t256_v40_peaky), by S > 1024 (t256_l512: 5 passes of the
                                   state loop; t256_max: Lmax 909, the gradient kernel at 65,484 B of LDS), and
                                   every wave-class case again under ctc_loss.wave = 0
  unsupported                      Lmax 910 (class -1, OS2S_ERR_UNSUPPORTED)
  ctc_log_softmax / ctc_grad / ctc_finish run in every case; blank = 0, grad_scale with a device factor,
  the bf16 gradient alone, in_len / label_len outside their ranges (the clamps) are variants.
Not reached: Lmax = 0 (a label tensor without columns has no address to pass); B * T of 2^31 / V rows and more
(the row index is 64-bit); V = 2.
w4_edges has 11 samples (the nine lengths of the table plus the tight and the infeasible-by-one sample).

Largest error / bound per stage over all cases and variants (CTC-RATIO lines; 0: bit-identical). The exact
checks (step 0, the growth of coff, valid, loglik and loss of infeasible samples, every +0, bf16 = rne(fp32), the
rerun on clean padding) are 0 on both backends.
                         logp  alpha.step beta.step loglik loss_per_sample loss_mean dlogits bf16 alone  end to end: loss dlogits
  fp32 torch emulation   0.43  0.70       0.73      0.38   0.72            0.39      0.13    0.95        0.61             0.64
  MI355X                 0.43  0.69       0.71      0.38   0.90            0.37      0.12    0.95        0.61             0.64
The end-to-end maxima are t256_max on both backends, to three digits the same: 909 labels and 29 repeats in 960
frames leave few alignments, the logsumexp terms vanish and the recursion is a chain of fp32 additions that the
emulation and the kernel round alike. There the states that reach the end run far below the row maximum a
renormalisation subtracts, so a step rounds a larger value than eight steps' growth of the log-likelihood; the
bound still holds with the margin shown. Every other case stays below 0.2 end to end.
Bounds that had to be completed: none; no constant of the issue's forms was changed and no run found a kernel bug.
Three checks were added to them: the growth of coff at a due renormalisation equals the fp32 row maximum of the
stored row (so "coff changes only where a renormalisation is due" is checked as an equality, the maximum being
negative as a rule); loglik is exactly 0 where a sample is infeasible; the bf16 gradient computed alone
(want_grad = False) is held to the fp32 bound plus 2^-8 relative for its one rounding and must equal bit for bit
the bf16 gradient of the run that also gives the fp32 one."""
import math
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
  sys.path.insert(0, REPO)

from _bn_cases import _Checks  # noqa: E402

U32 = 2.0 ** -24
NEG = float(torch.tensor(-1e30, dtype=torch.float32))     # kNegInf: the finite fp32 sentinel of a dead state
DEAD = -5e29                # entries <= DEAD are dead
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
K_TC = 32                   # kTC: time steps of log-probs per prefetch chunk
RENORM = 8                  # a renormalisation after every 8th step

# T, V, Lmax, logit scale, number of label symbols (None: V - 1), samples (T_b, L) and the class the table names.
# "tight" / "over": L = Lmax with T_b trimmed to L + repeats / to L + repeats - 1 (infeasible by one frame).
CASES = {
    "w4_edges": dict(T=40, V=5, Lmax=12, scale=2.0, alphabet=4, klass=4,
                     samples=[(40, 12), (1, 0), (1, 1), (8, 3), (9, 4), (32, 12), (33, 12), (40, 0), (31, 7),
                              "tight", "over"]),
    "w4_full": dict(T=300, V=29, Lmax=127, scale=3.0, klass=4, samples=[(300, 127), (280, 126), (131, 64)]),
    "w4_repeat": dict(T=200, V=3, Lmax=90, scale=4.0, alphabet=2, klass=4, samples=[(200, 90), (150, 61), (64, 21)]),
    "w8_lo": dict(T=280, V=29, Lmax=128, scale=3.0, klass=8, samples=[(280, 128), (270, 127), (33, 5)]),
    "w8_hi": dict(T=530, V=32, Lmax=255, scale=3.0, klass=8, samples=[(530, 255), (512, 200)]),
    "w8_repeat": dict(T=420, V=3, Lmax=200, scale=6.0, alphabet=2, klass=8, samples=[(420, 200), (353, 129)]),
    "w16_lo": dict(T=540, V=29, Lmax=256, scale=1.0, klass=16, samples=[(540, 256), (300, 130)]),
    "w16_hi": dict(T=1040, V=29, Lmax=511, scale=3.0, klass=16, samples=[(1040, 511), (1025, 257)]),
    "w16_repeat": dict(T=900, V=3, Lmax=511, scale=6.0, alphabet=2, klass=16, samples=[(900, 400)]),
    "t256_l512": dict(T=1040, V=29, Lmax=512, scale=3.0, klass=0, samples=[(1040, 512), (64, 9)]),
    "t256_v33": dict(T=300, V=33, Lmax=140, scale=3.0, klass=0, samples=[(300, 140), (290, 128), (17, 3)]),
    "t256_v40_peaky": dict(T=300, V=40, Lmax=140, scale=10.0, klass=0, vpad=40, samples=[(300, 140), (150, 60)]),
    "t256_max": dict(T=960, V=29, Lmax=909, scale=2.0, klass=0, samples=[(960, 909)]),
    "v5_peaky20": dict(T=400, V=5, Lmax=150, scale=20.0, klass=8, samples=[(400, 150), (333, 97)]),
}
WAVE_CASES = tuple(k for k, c in CASES.items() if c["klass"] > 0)
VARIANTS = {
    "base": list(CASES),
    "wave0": list(WAVE_CASES),                       # the 256-thread kernel on the same inputs, same bounds
    "blank0": ["w4_repeat", "w8_lo", "t256_v33"],
    "gscale": ["w4_edges", "t256_v33"],              # grad_scale = 1 / B, grad_scale_dev = [1024.]
    "bf16only": ["w8_lo"],                           # want_grad = False, the bf16 gradient only
    "clamp": ["w4_full"],                            # in_len = T + 5 and -1, label_len = Lmax + 3
}
PAIRS = [(c, v) for v, cs in VARIANTS.items() for c in cs]


def kernel_class_mirror(V, Lmax, wave=1):
  """Python mirror of os2s_ctc_loss_kernel_class (the library's own query is the authority on the GPU)."""
  Smax = 2 * Lmax + 1
  if Smax * 12 + K_TC * V * 4 > 65536 or Smax * 4 * 9 > 65536:
    return -1
  if wave and V <= 32:
    for ks in (4, 8, 16):
      if Smax <= 64 * ks:
        return ks
  return 0


def _repeats(lab):
  return int((lab[1:] == lab[:-1]).sum()) if lab.numel() > 1 else 0


def make_inputs(case, variant="base"):
  c = CASES[case]
  T, V, Lmax = c["T"], c["V"], c["Lmax"]
  blank = 0 if variant == "blank0" else V - 1
  lo = 1 if blank == 0 else 0                     # label symbols lo .. lo + alphabet - 1, never the blank
  nsym = c.get("alphabet") or V - 1
  g = torch.Generator().manual_seed(sum(map(ord, case)) * 7 + 1)
  B = len(c["samples"])
  labels = torch.zeros(B, Lmax, dtype=torch.int32)
  in_len, label_len, feasible = [], [], []
  for b, smp in enumerate(c["samples"]):
    Tb, L = (None, Lmax) if isinstance(smp, str) else smp
    while True:
      lab = torch.randint(lo, lo + nsym, (L,), generator=g, dtype=torch.int32)
      need = L + _repeats(lab)
      if Tb is None or need <= Tb:
        break
    if smp == "tight":
      Tb = need
    elif smp == "over":
      Tb = need - 1
    labels[b, :L] = lab
    labels[b, L:] = lab[L - 1] if L > 0 else lo
    in_len.append(Tb)
    label_len.append(L)
    feasible.append(Tb > 0 and need <= Tb)
  assert max(in_len) == T, case
  if variant == "clamp":
    in_len[0], label_len[0], in_len[2], feasible[2] = T + 5, Lmax + 3, -1, False
  in_len = torch.tensor(in_len, dtype=torch.int32)
  label_len = torch.tensor(label_len, dtype=torch.int32)
  clean = (torch.randn(T, B, V, generator=g) * c["scale"]).to(F32)
  dead = torch.arange(T)[:, None] >= in_len.long().clamp(0, T)[None, :]
  logits = torch.where(dead[:, :, None], torch.full_like(clean, math.nan), clean)
  clean = torch.where(dead[:, :, None], torch.zeros_like(clean), clean)
  inp = dict(case=case, variant=variant, T=T, B=B, V=V, Lmax=Lmax, blank=blank, logits=logits, clean=clean,
             in_len=in_len, labels=labels, label_len=label_len, feasible=torch.tensor(feasible),
             grad_scale=1.0, grad_scale_dev=None, want_grad=variant != "bf16only", want_bf16=True,
             vpad=c.get("vpad", 32 if V <= 32 else (V + 7) // 8 * 8), wave=0 if variant == "wave0" else 1)
  inp["klass"] = 0 if variant == "wave0" else c["klass"]
  if variant == "gscale":
    inp["grad_scale"], inp["grad_scale_dev"] = 1.0 / B, torch.tensor([1024.0], dtype=F32)
  return inp


def grad_scale_of(inp):
  """The fp32 factor the gradient kernel forms: fl(grad_scale) * (*grad_scale_dev)."""
  gs = torch.tensor(inp["grad_scale"], dtype=F32)
  if inp["grad_scale_dev"] is not None:
    gs = gs * inp["grad_scale_dev"][0]
  return gs


def geometry(inp):
  """The clamped lengths, the extended labels and the transition tables of a batch."""
  T, B, Lmax, blank = inp["T"], inp["B"], inp["Lmax"], inp["blank"]
  Smax = 2 * Lmax + 1
  Tb = inp["in_len"].long().clamp(0, T)
  L = inp["label_len"].long().clamp(0, Lmax)
  S = 2 * L + 1
  s = torch.arange(Smax)
  odd = (s & 1) == 1
  inS = s[None, :] < S[:, None]
  ext = torch.where(odd[None, :] & inS, inp["labels"].long()[:, (s >> 1).clamp(max=Lmax - 1)], blank)
  assert bool((ext[:, 1::2][inS[:, 1::2]] != blank).all())
  pad2 = torch.full((B, 2), -1, dtype=torch.long)
  same_prev = odd[None, :] & inS & (s[None, :] >= 3) & (torch.cat([pad2, ext[:, :-2]], 1) == ext)
  same_next = odd[None, :] & (s[None, :] + 2 < S[:, None]) & (torch.cat([ext[:, 2:], pad2], 1) == ext)
  rep = same_prev.sum(1)
  ok = (Tb > 0) & (L + rep <= Tb)
  skip_a = odd[None, :] & inS & (s[None, :] >= 3) & ~same_prev          # state s - 2 feeds s (alpha)
  skip_b = odd[None, :] & (s[None, :] + 2 < S[:, None]) & ~same_next     # state s + 2 feeds s (beta)
  return dict(T=T, B=B, V=inp["V"], Lmax=Lmax, Smax=Smax, Sld=(Smax + 15) & ~15, Tb=Tb, L=L, S=S, inS=inS, ext=ext,
              rep=rep, ok=ok, skip_a=skip_a, skip_b=skip_b, blank=blank)


def check_inputs(case, variant="base"):
  """Host-only conditions on a case's inputs: the feasibility the table intends, the class its shape reaches by
  the mirror of the dispatch, and for the *_repeat cases an allowed and a forbidden skip at a lane edge of the
  wave kernel in both directions (alpha: register 1 takes s - 2 from the previous lane; beta: register KS - 1
  takes s + 2 from the next lane)."""
  inp = make_inputs(case, variant)
  G = geometry(inp)
  assert torch.equal(G["ok"], inp["feasible"]), (case, G["ok"], inp["feasible"])
  assert kernel_class_mirror(inp["V"], inp["Lmax"], inp["wave"]) == inp["klass"], case
  if case == "w4_edges" and variant == "base":
    need = G["L"] + G["rep"]
    assert int(need[-2]) == int(G["Tb"][-2]) and int(need[-1]) == int(G["Tb"][-1]) + 1
  if case.endswith("_repeat"):
    ks = CASES[case]["klass"]
    s = torch.arange(G["Smax"])
    for tab, edge in ((G["skip_a"], (s % ks == 1) & (s >= 3)), (G["skip_b"], s % ks == ks - 1)):
      at = edge[None, :] & (s[None, :] + (0 if tab is G["skip_a"] else 2) < G["S"][:, None])
      assert bool((tab & at).any()) and bool((~tab & at).any()), case
  return inp, G


# ---------------------------------------------------------------------------------------------------------
# the CPU backend: the kernels' algorithm in torch, fp32 (or fp64), vectorised over the batch and the states
# ---------------------------------------------------------------------------------------------------------
MUTANTS = {
    # name: the case it runs on
    "skip_dropped_at_lane_edge": "w4_repeat",
    "skip_across_repeat": "w4_repeat",
    "beta_starts_at_last_state_only": "w4_edges",
    "renorm_not_in_coff": "w4_edges",
    "stale_prefetch_row": "w4_edges",
    "states_from_256_never_updated": "t256_v33",
    "blank_occupancy_over_odd_states": "w4_edges",
    "bf16_truncated": "w4_edges",
    "infeasible_by_one_valid": "w4_edges",
    "dead_frame_softmax": "w4_edges",
}


class Emu:
  """The algorithm of csrc/ctc_loss.hip: log-softmax, the alpha / beta recursions with a renormalisation after
  every 8th step (the normaliser kept in double, the finite sentinel -1e30), the gradient, the finish. Rows and
  coff are stored as the kernels store them. dtype F64: the same algorithm without fp32 rounding."""

  def __init__(self, dtype=F32, mutant=None):
    self.dt, self.mutant = dtype, mutant

  def _lse3(self, a0, a1, a2):
    m = torch.maximum(a0, torch.maximum(a1, a2))
    v = m + torch.log(torch.exp(a0 - m) + torch.exp(a1 - m) + torch.exp(a2 - m))
    return torch.where(m <= DEAD, torch.full_like(v, NEG), v)

  def _recursion(self, logp, G, ok, beta):
    dt, mut = self.dt, self.mutant
    B, T, Smax, Sld, Tb, S = G["B"], G["T"], G["Smax"], G["Sld"], G["Tb"], G["S"]
    neg = torch.full((B, Smax), NEG, dtype=dt)
    out = torch.full((B, T, Sld), math.nan, dtype=dt)
    coff = torch.full((B, T), math.nan, dtype=F64)
    C = torch.zeros(B, dtype=F64)
    cur = neg.clone()
    s = torch.arange(Smax)[None, :]
    skip = (G["skip_b"] if beta else G["skip_a"]).clone()
    if mut == "skip_dropped_at_lane_edge" and not beta:
      cand = (skip[0] & (s[0] % 4 == 1)).nonzero()
      skip[0, int(cand[len(cand) // 2])] = False
    if mut == "skip_across_repeat":
      odd = (s & 1) == 1
      skip = odd & ((s + 2 < S[:, None]) if beta else ((s >= 3) & G["inS"]))
    if beta:
      start = (s >= S[:, None] - (1 if mut == "beta_starts_at_last_state_only" else 2)) & G["inS"]
    else:
      start = (s <= 1) & G["inS"]
    ar = torch.arange(B)
    fill1, fill2 = neg[:, :1], neg[:, :2]
    for k in range(int(Tb[ok].max()) if bool(ok.any()) else 0):
      act = ok & (k < Tb)
      t = ((Tb - 1 - k) if beta else torch.full_like(Tb, k)).clamp(0, T - 1)
      kl = k - 1 if (mut == "stale_prefetch_row" and k == K_TC) else k
      tl = ((Tb - 1 - kl) if beta else torch.full_like(Tb, kl)).clamp(0, T - 1)
      lpe = logp[ar, tl].gather(1, G["ext"])
      if k == 0:
        v = torch.where(start, lpe, neg)
      else:
        if beta:
          a1, a2 = torch.cat([cur[:, 1:], fill1], 1), torch.cat([cur[:, 2:], fill2], 1)
        else:
          a1, a2 = torch.cat([fill1, cur[:, :-1]], 1), torch.cat([fill2, cur[:, :-2]], 1)
        v = self._lse3(cur, a1, torch.where(skip, a2, neg)) + lpe
        v = torch.where(v < NEG, neg, v)
      v = torch.where(G["inS"], v, neg)
      if mut == "states_from_256_never_updated":
        v = torch.where(s >= 256, neg, v)
      cur = torch.where(act[:, None], v, cur)
      ia = act.nonzero()[:, 0]
      out[ia, t[ia], :Smax] = cur[ia]
      coff[ia, t[ia]] = C[ia]
      if k % RENORM == RENORM - 1:
        m = cur.max(1).values
        do = act & (k + 1 < Tb) & (m > DEAD)
        cur = torch.where(do[:, None], torch.where(cur > DEAD, cur - m[:, None], neg), cur)
        if mut != "renorm_not_in_coff":
          C = C + torch.where(do, m.double(), torch.zeros_like(C))
    return out, coff, C, cur

  def run(self, inp):
    dt, mut = self.dt, self.mutant
    G = geometry(inp)
    B, T, V, Tb, S = G["B"], G["T"], G["V"], G["Tb"], G["S"]
    live = (torch.arange(T)[None, :] < Tb[:, None])                     # [B,T]
    x = inp["logits"].permute(1, 0, 2).to(dt)
    m = x.max(-1, keepdim=True).values
    logp = x - (m + torch.log(torch.exp(x - m).sum(-1, keepdim=True)))
    logp = torch.where(live[:, :, None], logp, torch.full_like(logp, math.nan))
    ok = G["ok"] if mut != "infeasible_by_one_valid" else (Tb > 0) & (G["L"] + G["rep"] <= Tb + 1)
    alpha, coff_a, C, last = self._recursion(logp, G, ok, False)
    beta, coff_b, _, _ = self._recursion(logp, G, ok, True)
    ar = torch.arange(B)
    l1 = last[ar, S - 1]
    l2 = torch.where(S >= 2, last[ar, (S - 2).clamp(min=0)], torch.full_like(l1, NEG))
    mm = torch.maximum(l1, l2)
    lse = torch.where(mm <= DEAD, torch.full_like(mm, NEG), mm + torch.log(torch.exp(l1 - mm) + torch.exp(l2 - mm)))
    lse = torch.where(S >= 2, lse, l1)
    valid = ok & (lse > DEAD)
    if mut == "infeasible_by_one_valid":
      valid = ok
    loglik = torch.where(ok, C + lse.double(), torch.zeros(B, dtype=F64))
    loss = torch.where(valid, (-loglik).to(dt), torch.zeros(B, dtype=dt))
    loss = torch.where(torch.isfinite(loss), loss, torch.zeros_like(loss))
    tot = torch.zeros((), dtype=dt)
    for b in range(B):
      tot = tot + loss[b]
    res = dict(logp=logp.to(F32 if dt is F32 else F64), alpha=alpha, beta=beta, coff_a=coff_a, coff_b=coff_b,
               loglik=loglik, valid=valid.to(torch.int32), loss_per_sample=loss, loss_mean=(tot / B).reshape(1),
               dlogits=None, dlogits_bf16=None)
    # gradient
    gs = grad_scale_of(inp).to(dt)
    Smax = G["Smax"]
    lpe = logp.gather(2, G["ext"][:, None, :].expand(B, T, Smax))
    off = (coff_a + coff_b - loglik[:, None]).to(dt)
    e = (alpha[:, :, :Smax] + beta[:, :, :Smax] - lpe) + off[:, :, None]
    use = live[:, :, None] & valid[:, None, None] & G["inS"][:, None, :]
    e = torch.where(use & (e > -80.0), torch.exp(e), torch.zeros_like(e))
    idx = G["ext"][:, None, :].expand(B, T, Smax)
    if mut == "blank_occupancy_over_odd_states":
      odd = (torch.arange(Smax) & 1) == 1
      occ_b = torch.where(odd[None, None, :], e, torch.zeros_like(e)).sum(-1)
      e = torch.where(odd[None, None, :], e, torch.zeros_like(e))
      occ = torch.zeros(B, T, V, dtype=dt).scatter_add_(2, idx, e)
      occ[:, :, G["blank"]] = occ_b
    else:
      occ = torch.zeros(B, T, V, dtype=dt).scatter_add_(2, idx, e)
    gl = live[:, :, None] & valid[:, None, None]
    g = torch.where(gl, (torch.exp(logp) - occ) * gs, torch.zeros(B, T, V, dtype=dt))
    if mut == "dead_frame_softmax":
      g = torch.where(gl, g, torch.full_like(g, 1.0 / V) * gs)
    g16 = torch.zeros(B, T, inp["vpad"], dtype=BF16)
    if mut == "bf16_truncated":
      g16[:, :, :V] = (g.float().contiguous().view(torch.int32) & -65536).view(F32).to(BF16)
    else:
      g16[:, :, :V] = g.float().to(BF16)
    if inp["want_grad"]:
      res["dlogits"] = g.permute(1, 0, 2).contiguous()
    if inp["want_bf16"]:
      res["dlogits_bf16"] = g16
    return res


# ---------------------------------------------------------------------------------------------------------
# the stages
# ---------------------------------------------------------------------------------------------------------
class _Run:
  def __init__(self, name, log):
    self.name, self.log, self.ratios, self.fails = name, log, {}, []

  def within(self, stage, got, ref, bound, mask=None):
    if mask is not None:
      z = torch.zeros((), dtype=F64)
      mask = mask.expand_as(got)
      got, ref, bound = (torch.where(mask, v.to(F64).expand_as(got), z) for v in (got, ref, bound))
    chk = _Checks()
    chk.within(stage, got, ref, bound)
    self._take(chk)

  def bits(self, stage, got, ref, mask=None):
    chk = _Checks()
    chk.bits(stage, got, ref, mask)
    self._take(chk)

  def true(self, stage, cond, what=""):
    self.ratios.setdefault(stage, 0.0)
    if not bool(cond):
      self.ratios[stage] = math.inf
      self.fails.append("%s %s: %s" % (self.name, stage, what or "does not hold"))

  def _take(self, chk):
    for k, v in chk.ratios.items():
      self.ratios[k] = max(self.ratios.get(k, 0.0), v)
    self.fails.extend("%s %s" % (self.name, f) for f in chk.fails)

  def report(self):
    for k in sorted(self.ratios):
      self.log("CTC-RATIO %-26s %-40s %.3g" % (self.name, k, self.ratios[k]))
    for f in self.fails:
      self.log("CTC-FAIL " + f)


def _cmp_logp(run, R, inp, G):
  # lz = m + log(sum_v exp(x_v - m)), logp = x - lz. The subtraction x - m is exact to u32 |x - m|, which exp turns
  # into a relative error of the term; V accurate exps and a V-term sum give (V + 2) u32 relative to the sum, that
  # is absolute in its logarithm; logf adds 1 ulp, m + log s rounds to u32 |lz|, x - lz to u32 |ref|: with the
  # margin of the issue's form, u32 (V + 4 + 2 |lz| + 2 |ref|).
  x = inp["clean"].permute(1, 0, 2).double()
  lz = torch.logsumexp(x, -1, keepdim=True)
  ref = x - lz
  live = (torch.arange(G["T"])[None, :] < G["Tb"][:, None])[:, :, None]
  run.within("logp", R["logp"], ref, U32 * (G["V"] + 4 + 2 * lz.abs() + 2 * ref.abs()), live)


def _cmp_recursion(run, R, G, beta):
  # One step, vectorised over every (sample, step >= 1, state < S). The row the kernel held is the stored row of the
  # previous step minus the growth of the double normaliser (the fp32 row maximum a renormalisation subtracted; that
  # subtraction rounds to u32 |entry| / 2). lse3 of at most three live entries: the scaled differences, two exp2,
  # the sum, log2 and the product with ln 2 stay below 16 u32 absolute (2 ulp each for exp2 / log2 on values
  # <= 1 / <= 1.6); max + ..., + logp round relative to the magnitudes involved: u32 (16 + 4 max(|live
  # predecessors|, |expected|)). A state without a live predecessor holds the sentinel itself.
  name = "beta" if beta else "alpha"
  B, T, Smax, Tb, S, V = G["B"], G["T"], G["Smax"], G["Tb"], G["S"], G["V"]
  ok = G["ok"]
  k = torch.arange(T)[None, :]
  tk = ((Tb[:, None] - 1 - k) if beta else k.expand(B, T)).clamp(0, T - 1)             # [B,T] time of step k
  step_live = (k < Tb[:, None]) & ok[:, None]
  X = R[name].gather(1, tk[:, :, None].expand(B, T, R[name].shape[2]))[:, :, :Smax]   # step-ordered rows
  Ck = R["coff_b" if beta else "coff_a"].gather(1, tk)
  lpe = R["logp"].gather(1, tk[:, :, None].expand(B, T, V)).double().gather(2, G["ext"][:, None, :].expand(B, T, Smax))
  inS = G["inS"][:, None, :]
  s = torch.arange(Smax)[None, None, :]
  Xd = X.double()
  # step 0: the initial condition, copied bits of logp / the sentinel itself
  start = ((s >= S[:, None, None] - 2) if beta else (s <= 1)) & inS
  m0 = (step_live[:, :1, None] & inS)
  ref0 = torch.where(start[:, 0], lpe[:, 0], torch.full_like(lpe[:, 0], NEG))
  run.within(name + ".step0 (exact)", Xd[:, 0], ref0, torch.zeros_like(ref0), m0[:, 0])
  # the normaliser: 0 at step 0, changed only by a due renormalisation (after step k - 1 = 7 mod 8, k < T_b), and
  # then by the fp32 row maximum of step k - 1
  dC = Ck[:, 1:] - Ck[:, :-1]
  due = ((k[:, 1:] % RENORM) == 0) & step_live[:, 1:]
  run.within("coff_%s.step0 (exact)" % name[0], Ck[:, 0], torch.zeros(B, dtype=F64), torch.zeros(B, dtype=F64),
             step_live[:, 0])
  rowmax = torch.where(inS & (Xd > DEAD), Xd, torch.full_like(Xd, -math.inf)).max(-1).values[:, :-1]
  want = torch.where(due & torch.isfinite(rowmax), rowmax, torch.zeros_like(rowmax))
  run.within("coff_%s.growth" % name[0], dC, want, 1e-12 * (1.0 + Ck[:, 1:].abs()), step_live[:, 1:])
  # steps >= 1
  prev = Xd[:, :-1] - dC[:, :, None]
  prev = torch.where((Xd[:, :-1] > DEAD) & inS, prev, torch.full_like(prev, -math.inf))
  ninf1 = torch.full((B, T - 1, 1), -math.inf, dtype=F64)
  if beta:
    p1 = torch.cat([prev[:, :, 1:], ninf1], 2)
    p2 = torch.cat([prev[:, :, 2:], ninf1, ninf1], 2)
    skip = G["skip_b"]
  else:
    p1 = torch.cat([ninf1, prev[:, :, :-1]], 2)
    p2 = torch.cat([ninf1, ninf1, prev[:, :, :-2]], 2)
    skip = G["skip_a"]
  p2 = torch.where(skip[:, None, :], p2, torch.full_like(p2, -math.inf))
  P = torch.stack([prev, p1, p2], 0)
  lse = torch.logsumexp(P, 0)
  alive = torch.isfinite(lse)
  exp_v = lse + lpe[:, 1:]
  mag = torch.where(torch.isfinite(P), P.abs(), torch.zeros_like(P)).max(0).values
  mag = torch.maximum(mag, torch.where(alive, exp_v.abs(), torch.zeros_like(exp_v)))
  mask = step_live[:, 1:, None] & inS
  got = Xd[:, 1:]
  run.within(name + ".step", got, torch.where(alive, exp_v, torch.full_like(exp_v, NEG)),
             torch.where(alive, U32 * (16 + 4 * mag), torch.zeros_like(mag)), mask)


def _cmp_loglik(run, R, inp, G):
  # l2 = lse2 of the last two states of the last row (one state for L = 0): exp(0) = 1, one __expf of a value <= 1,
  # the sum, __logf of [1, 2]: below 4 u32; max + ... rounds to u32 |l2|, the fp64 sum with the normaliser is exact
  # to 2^-53: u32 (4 + 2 |l2|).
  B, Tb, S, ok = G["B"], G["Tb"], G["S"], G["ok"]
  ar = torch.arange(B)
  tl = (Tb - 1).clamp(min=0)
  row = R["alpha"][ar, tl].double()
  a1 = row[ar, S - 1]
  a2 = torch.where(S >= 2, row[ar, (S - 2).clamp(min=0)], torch.full_like(a1, -math.inf))
  a1 = torch.where(a1 > DEAD, a1, torch.full_like(a1, -math.inf))
  a2 = torch.where(a2 > DEAD, a2, torch.full_like(a2, -math.inf))
  l2 = torch.logsumexp(torch.stack([a1, a2]), 0)
  ref = R["coff_a"][ar, tl] + l2
  valid = R["valid"] != 0
  run.true("valid = feasible", torch.equal(valid, ok), "valid %s, feasible %s" % (valid.tolist(), ok.tolist()))
  run.within("loglik", R["loglik"], ref, U32 * (4 + 2 * l2.abs()), ok & valid)
  zero = torch.zeros(B, dtype=F64)
  run.within("loglik: 0 where not feasible (exact)", R["loglik"], zero, zero, ~ok)
  # loss_per_sample = fl32(-loglik): one rounding, u32 |loglik|; exactly 0 where not valid
  ll = R["loglik"]
  run.within("loss_per_sample", R["loss_per_sample"], -ll, U32 * ll.abs(), valid)
  run.bits("loss_per_sample: +0 where not valid", R["loss_per_sample"].float(), torch.zeros(B), ~valid)
  # loss_mean: B fp32 additions and a division of the backend's own losses: B u32 mean|loss|
  lps = R["loss_per_sample"].double()
  run.within("loss_mean", R["loss_mean"], lps.sum().reshape(1) / B, B * U32 * lps.abs().mean().reshape(1))


def _cmp_grad(run, R, inp, G):
  # g = gs (p - occ_v), p = exp(logp), occ_v = sum_{s: l'_s = v} e_s, e_s = exp(x_s), x_s = (alpha + beta - logp) +
  # off, off = fl32(coff_a + coff_b - loglik). x_s carries 4 roundings of magnitudes <= X = |alpha| + |beta| +
  # |logp| + |off|: 4 u32 X absolute, which __expf (its own scaling by log2 e: another u32 |x| <= u32 X, and 2 ulp)
  # turns into e_s (8 X + 4) u32 relative; summed over the class's states: occ (8 X_t + 4) u32, X_t the largest X
  # of the frame's states above the -80 flush. The <= S / 2-term fp32 sum of terms <= 1 whose total is <= 1 adds at
  # most S u32 / 2, the flush e^-80 S nothing; p = __expf(logp): (|logp| + 3) u32 relative; the subtraction and the
  # product with gs 2 u32 of <= 2: gs u32 [(S + 8) + occ (8 X_t + 4) + p (|logp| + 3)].
  B, T, V, Smax, Tb, S = G["B"], G["T"], G["V"], G["Smax"], G["Tb"], G["S"]
  valid = R["valid"] != 0
  gs = float(grad_scale_of(inp))
  live = (torch.arange(T)[None, :] < Tb[:, None]) & valid[:, None]                      # [B,T]
  use = live[:, :, None] & G["inS"][:, None, :]
  z3 = torch.zeros(B, T, Smax, dtype=F64)
  lp = torch.where(live[:, :, None], R["logp"].double(), torch.zeros(B, T, V, dtype=F64))
  idx = G["ext"][:, None, :].expand(B, T, Smax)
  lpe = lp.gather(2, idx)
  al = torch.where(use, R["alpha"][:, :, :Smax].double(), z3)
  be = torch.where(use, R["beta"][:, :, :Smax].double(), z3)
  off = torch.where(live, R["coff_a"] + R["coff_b"] - R["loglik"][:, None], torch.zeros(B, T, dtype=F64))[:, :, None]
  x = torch.where(use, al + be - lpe + off, torch.full_like(z3, -math.inf))
  e = torch.exp(x)
  X = torch.where(x > -80.0, al.abs() + be.abs() + lpe.abs() + off.abs(), z3).max(-1).values[:, :, None]
  occ = torch.zeros(B, T, V, dtype=F64).scatter_add_(2, idx, e)
  p = torch.exp(lp)
  ref = torch.where(live[:, :, None], gs * (p - occ), torch.zeros(B, T, V, dtype=F64))
  bound = gs * U32 * ((S[:, None, None] + 8).double() + occ * (8 * X + 4) + p * (lp.abs() + 3))
  bound = torch.where(live[:, :, None], bound, torch.zeros_like(bound))
  ref, bound = ref.permute(1, 0, 2), bound.permute(1, 0, 2)
  livet = live.t()[:, :, None]
  if R["dlogits"] is not None:
    g = R["dlogits"]
    run.within("dlogits", g, ref, bound)
    run.bits("dlogits: +0 at t >= in_len and where not valid", g.float(), torch.zeros(T, B, V), ~livet)
  g16 = R["dlogits_bf16"]
  if g16 is not None:
    vpad = g16.shape[2]
    if R["dlogits"] is not None:
      # the convert is round-to-nearest-even of the fp32 gradient: the same bits
      run.bits("dlogits_bf16 = rne(dlogits)", g16[:, :, :V].contiguous(),
               R["dlogits"].float().permute(1, 0, 2).to(BF16).contiguous())
    else:
      # alone: the rounded fp32 value, 2^-8 relative on top of the fp32 bound
      rb, bb = ref.permute(1, 0, 2), bound.permute(1, 0, 2)
      run.within("dlogits_bf16 (alone)", g16[:, :, :V], rb, bb * (1 + 2.0 ** -8) + 2.0 ** -8 * rb.abs())
      run.bits("dlogits_bf16: +0 at t >= in_len and where not valid", g16[:, :, :V].contiguous(),
               torch.zeros(B, T, V, dtype=BF16), ~live[:, :, None])
    if vpad > V:
      run.bits("dlogits_bf16: +0 in the padded columns", g16[:, :, V:].contiguous(),
               torch.zeros(B, T, vpad - V, dtype=BF16))


_REF = {}


def reference(case, variant):
  """(loss [B], dlogits [T,B,V]) of oracle.ctc.ctc_loss_torch in float64 for the unit gradient scale; computed
  once per set of inputs and shared."""
  key = (case, "base" if variant in ("wave0", "gscale", "bf16only") else variant)
  if key not in _REF:
    from oracle import ctc
    inp = make_inputs(*key)
    G = geometry(inp)
    loss, _, grad = ctc.ctc_loss_torch(inp["clean"], G["Tb"], inp["labels"], G["L"], blank=inp["blank"], want_grad=True,
                                       dtype=F64)
    _REF[key] = (loss, grad)
  return _REF[key]


def _cmp_end_to_end(run, R, inp, G):
  # Against the independent float64 oracle, per valid sample. Each of the T_b steps rounds twice a value no larger
  # than the growth since the last renormalisation, at most 8 steps' worth of the log-likelihood:
  # |loss - ref| <= u32 (16 |ref| + 8 T_b); a gradient element is a posterior <= 1 formed from alpha + beta - loglik,
  # each within that bound, plus the gradient stage's own u32 (S + 16).
  ref_loss, ref_grad = reference(inp["case"], inp["variant"])
  ok, Tb, S = G["ok"], G["Tb"], G["S"]
  gs = float(grad_scale_of(inp))
  lb = U32 * (16 * ref_loss.abs() + 8 * Tb.double())
  run.within("end to end: loss", R["loss_per_sample"], ref_loss, lb, ok)
  gb = gs * (lb + U32 * (S.double() + 16))[None, :, None]
  live = ((torch.arange(G["T"])[:, None] < Tb[None, :]) & ok[None, :])[:, :, None]
  if R["dlogits"] is not None:
    run.within("end to end: dlogits", R["dlogits"], gs * ref_grad, gb, live)


def check_case(case, variant, be, log=print, tag=None):
  """Walks one (case, variant) through every stage on backend `be`; returns dict(fails, ratios, out). fails is
  empty iff every output kept its bound."""
  inp, G = check_inputs(case, variant)
  run = _Run(tag or "%s/%s" % (case, variant), log)
  if variant == "bf16only":
    R0 = be.run(inp)
    assert R0["dlogits"] is None and R0["dlogits_bf16"] is not None
    _cmp_grad(run, R0, inp, G)
    inp = dict(inp, want_grad=True)
    R = be.run(inp)
    run.bits("bf16 alone = bf16 beside the fp32 gradient", R0["dlogits_bf16"], R["dlogits_bf16"])
    run.bits("loss unchanged by want_grad", R0["loss_per_sample"].float(), R["loss_per_sample"].float())
  else:
    R = be.run(inp)
  _cmp_logp(run, R, inp, G)
  _cmp_recursion(run, R, G, False)
  _cmp_recursion(run, R, G, True)
  _cmp_loglik(run, R, inp, G)
  _cmp_grad(run, R, inp, G)
  _cmp_end_to_end(run, R, inp, G)
  # what the frames t >= in_len hold is never read: zeros in place of the NaNs give the same bits
  R2 = be.run(dict(inp, logits=inp["clean"]))
  for k in ("loss_per_sample", "loss_mean", "dlogits", "dlogits_bf16"):
    if R[k] is not None:
      a, b = (v.float() if v.dtype is F64 else v for v in (R[k], R2[k]))
      run.bits("rerun on clean padding: " + k, a.contiguous(), b.contiguous())
  run.report()
  return dict(fails=run.fails, ratios=run.ratios, out=R)
