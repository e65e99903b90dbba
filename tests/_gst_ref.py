"""Float64 references for the kernel-level tests of csrc/gst.hip and csrc/conv2d_toeplitz.hip
(tests/test_oracle_gst.py, tests/test_gst_kernels_gpu.py, tests/test_conv2d_toeplitz_gpu.py). Plain torch
on the CPU; every function takes the bf16 / fp32 tensors the kernel takes and casts them up. Nothing
here imports openseq2seq_amd."""
import torch

F64 = torch.float64


def _d(t):
  return t.detach().cpu().to(F64)


def gru_tf_ref(gxg, gxc, wgh, wch, lens, dh_final=None):
  """tf GRUCell under dynamic_rnn(sequence_length) on precomputed input projections.

  gxg [B,T,2H] = x Wg_x + bg (r | u), gxc [B,T,H] = x Wc_x + bc, wgh [H,2H], wch [H,H] ([in, out]),
  lens [B] int or None (= T everywhere); len = clamp(lens, 0, T). Per step
      ru = sigmoid(gxg_t + h wgh), r = ru[:, :H], u = ru[:, H:]
      c = tanh(gxc_t + (r*h) wch),  h' = u*h + (1-u)*c,
  the state carried unchanged through t >= len. Returns a dict of float64 tensors: h_seq [B,T+1,H],
  r, u, c, hprev (= h_{t-1}), rh (= r*h_{t-1}) [B,T,H] and h_final [B,H]; rows with t >= len hold
  r = 0, u = 1, c = 0, hprev = 0, rh = 0 (what the kernel documents). With dh_final [B,H] also dgxg and
  dgxc, by autograd through this same recurrence (zero at t >= len)."""
  gxg, gxc, wgh, wch = _d(gxg), _d(gxc), _d(wgh), _d(wch)
  B, T, H2 = gxg.shape
  H = H2 // 2
  if lens is None:
    ln = torch.full((B,), T, dtype=torch.int64)
  else:
    ln = torch.as_tensor(lens).detach().cpu().to(torch.int64).clamp(0, T)
  grad = dh_final is not None
  if grad:
    gxg.requires_grad_(True)
    gxc.requires_grad_(True)
  h = torch.zeros(B, H, dtype=F64)
  hs, rs, us, cs, hps, rhs = [h], [], [], [], [], []
  for t in range(T):
    live = (t < ln)[:, None]
    ru = torch.sigmoid(gxg[:, t] + h @ wgh)
    r, u = ru[:, :H], ru[:, H:]
    rh = r * h
    c = torch.tanh(gxc[:, t] + rh @ wch)
    hn = u * h + (1 - u) * c
    zero, one = torch.zeros_like(r), torch.ones_like(r)
    rs.append(torch.where(live, r, zero))
    us.append(torch.where(live, u, one))
    cs.append(torch.where(live, c, zero))
    hps.append(torch.where(live, h, zero))
    rhs.append(torch.where(live, rh, zero))
    h = torch.where(live, hn, h)
    hs.append(h)
  out = dict(h_seq=torch.stack(hs, 1), r=torch.stack(rs, 1), u=torch.stack(us, 1), c=torch.stack(cs, 1),
             hprev=torch.stack(hps, 1), rh=torch.stack(rhs, 1), h_final=h)
  if grad:
    dgxg, dgxc = torch.autograd.grad(h, [gxg, gxc], _d(dh_final), allow_unused=True)
    out["dgxg"] = dgxg if dgxg is not None else torch.zeros(B, T, 2 * H, dtype=F64)
    out["dgxc"] = dgxc if dgxc is not None else torch.zeros(B, T, H, dtype=F64)
  return {k: v.detach() for k, v in out.items()}


def token_attention_ref(q, k, v, att_v, heads, dout=None):
  """Multi-head "bahdanau" token attention: q [B, heads*dh], k / v [N, heads*dh], att_v [dh]:
      w[b,h,n] = softmax_n sum_d tanh(att_v[d] * tanh(k[n,h,d] + q[b,h,d])),  out[b,h,:] = sum_n w v[n,h,:].
  Returns a dict of float64 tensors out [B, heads*dh], w [B, heads, N] and, with dout [B, heads*dh],
  dq, dk, dv, datt_v by autograd."""
  q, k, v, att_v = _d(q), _d(k), _d(v), _d(att_v)
  B, D = q.shape
  N = k.shape[0]
  dh = D // heads
  leaves = [q, k, v, att_v]
  if dout is not None:
    for t in leaves:
      t.requires_grad_(True)
  q4 = q.view(B, 1, heads, dh)
  k4 = k.view(1, N, heads, dh)
  s = torch.tanh(att_v * torch.tanh(k4 + q4)).sum(-1)          # [B, N, heads]
  w = torch.softmax(s, 1).permute(0, 2, 1)                      # [B, heads, N]
  o = torch.einsum("bhn,nhd->bhd", w, v.view(N, heads, dh)).reshape(B, D)
  out = dict(out=o, w=w)
  if dout is not None:
    gs = torch.autograd.grad(o, leaves, _d(dout))
    out.update(dq=gs[0], dk=gs[1], dv=gs[2], datt_v=gs[3])
  return {k_: v_.detach() for k_, v_ in out.items()}


def toeplitz_expand_ref(w, Fi, Fo, sF, padF):
  """w [KT,KF,Cin,Cout] -> W' [KT, Fo*Cout, Fi*Cin] (dtype of w) in the layout of conv2d_toeplitz.hip:
      W'[kt][(fo,co)][(fi,ci)] = w[kt][fi - fo*sF + padF][ci][co],  +0 outside the band."""
  KT, KF, Cin, Cout = w.shape
  out = torch.zeros(KT, Fo, Cout, Fi, Cin, dtype=w.dtype)
  for fo in range(Fo):
    for fi in range(Fi):
      kf = fi - fo * sF + padF
      if 0 <= kf < KF:
        out[:, fo, :, fi, :] = w[:, kf].transpose(1, 2)          # [KT,Cin,Cout] -> [KT,Cout,Cin]
  return out.reshape(KT, Fo * Cout, Fi * Cin)


def toeplitz_reduce_ref(dwexp, KF, Cin, Cout, Fi, Fo, sF, padF):
  """Adjoint of toeplitz_expand_ref: dwexp [KT, Fo*Cout, Fi*Cin] -> dw [KT,KF,Cin,Cout],
      dw[kt][kf][ci][co] = sum_fo dwexp[kt][(fo,co)][(fo*sF + kf - padF, ci)]."""
  KT = dwexp.shape[0]
  g = dwexp.reshape(KT, Fo, Cout, Fi, Cin)
  dw = torch.zeros(KT, KF, Cin, Cout, dtype=dwexp.dtype)
  for kf in range(KF):
    for fo in range(Fo):
      fi = fo * sF + kf - padF
      if 0 <= fi < Fi:
        dw[:, kf] += g[:, fo, :, fi, :].transpose(1, 2)
  return dw


def toeplitz_geometry(Fi, KF, sF, padding):
  """(Fo, padF) of the frequency axis: TF 'SAME' (the odd pad element goes to the right) or 'VALID'."""
  if padding == "SAME":
    Fo = -(-Fi // sF)
    total = max((Fo - 1) * sF + KF - Fi, 0)
    return Fo, total // 2
  return (Fi - KF) // sF + 1, 0


# (KT, KF, Cin, Cout, Fi, sF, padding): Fi*Cin and Fo*Cout are multiples of 8, as Conv2dBN requires
TOEPLITZ_CASES = [
    (3, 3, 1, 8, 16, 2, "SAME"),     # the style encoder's first layer: padF = 0, pad on the right only
    (3, 3, 8, 8, 7, 2, "SAME"),      # odd Fi, symmetric pad
    (2, 4, 2, 4, 12, 1, "SAME"),     # even KF, stride 1
    (5, 5, 2, 8, 12, 2, "VALID"),    # Fo = 4
    (1, 1, 8, 8, 4, 1, "SAME"),      # degenerate band
    (3, 41, 1, 8, 32, 2, "SAME"),    # DS2's 41-wide band on F = 32: KF > Fi
]
