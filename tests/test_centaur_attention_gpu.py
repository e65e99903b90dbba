"""The dense wide-head cross-attention of Centaur (csrc/attention_wide.hip: os2s_attention_wide_fwd /
os2s_attention_wide_bwd) against a float64 model written here.

Cases: forward and backward at D in {32, 512}, forward only at D in {64, 128, 256}; H in {1, 2}; B = 3; Tq in
{1, 7, 70} (70 crosses the 64-row tile); S in {8, 72} with (S, 1, S - 3) real keys, the rest carrying the -1e9 padding
bias; keep in {1.0, 0.9} with the mask rebuilt through capi.dropout_mask (element ((b*H + h)*Tq + t)*S + key). q, k
and v are column slices of wider tensors, the gradients go into column slices of buffers pre-filled with 7.0 whose
neighbouring columns must stay 7.0. The window cases put a window inside the source, across the last real key,
wholly past it (the near-uniform row of the additive fp32 bias: the model adds the bias in fp32 as the kernel's
contract says) and back_step 1 at position 0. argmax is exact wherever the float64 top-1 / top-2 gap exceeds 1e-2, a
second identical call is bitwise equal, unsupported D and S give OS2S_ERR_UNSUPPORTED (NotImplementedError from the
layer).

Bounds. The error of a tensor is max |got - ref| / (rms(ref) + |ref|). For o, dq, dk, dv the bound is twice the error
of the SAME float64 model with bf16 rounding at the kernel's documented rounding points (P o m / keep, dS, and the
four outputs), computed per case in the test. p is fp32 and never rounded, so its bound comes from the format: p =
exp(x - lse), so its relative error is at most twice the error of a logit, bounded by the fp32 dot-product bound
D * 2^-24 * scale * sum_d |q_d k_d| (largest of the case), plus 1e-5 for the exponential and the normalisation
(absolute floor 1e-9).

S in {256, 264, 512} (test_long_sources) is added to the cases above for the two row-pass mappings on either side of
S = 256 and for the largest LDS request.

Measured on an MI355X, the largest error over the cases of a head dim and the bound of that case (the tests print
every figure before they assert):

  D    H   o               dq              dk              dv              p (share of its bound)
  32   1   4.8e-3 (9.5e-3) 9.3e-3 (1.9e-2) 9.2e-3 (1.8e-2) 4.8e-3 (9.7e-3) 0.022
  32   2   4.6e-3 (9.2e-3) 1.4e-2 (2.9e-2) 1.0e-2 (2.0e-2) 5.9e-3 (1.2e-2) 0.028
  512  1   8.6e-3 (1.7e-2) 1.5e-2 (2.9e-2) 1.2e-2 (2.3e-2) 6.0e-3 (1.2e-2) 0.0010
  512  2   5.4e-3 (1.1e-2) 1.7e-2 (3.4e-2) 1.1e-2 (2.2e-2) 5.7e-3 (1.1e-2) 0.0012
  64   1/2 4.8e-3 / 5.6e-3 (9.7e-3 / 1.1e-2)                               0.010 / 0.011
  128  1/2 4.7e-3 / 5.3e-3 (9.5e-3 / 1.1e-2)                               0.0056 / 0.0059
  256  1/2 5.3e-3 / 7.0e-3 (1.1e-2 / 1.4e-2)                               0.0020 / 0.0030
  long sources, D 32:  o 3.0e-3 (6.1e-3), dq 7.2e-3 (1.4e-2), dk 1.2e-2 (2.3e-2), dv 4.7e-3 (9.5e-3), p 0.020
  long sources, D 512: o 3.9e-3 (7.9e-3), dq 8.4e-3 (1.7e-2), dk 1.2e-2 (2.5e-2), dv 5.3e-3 (1.1e-2), p 0.0013

In every row the device's largest error IS the rounded model's (the bound is exactly twice it): the worst element is
set by the bf16 roundings, which the device performs on the same values.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 3
TQS = [1, 7, 70]
SS = [8, 72]
KEEPS = [1.0, 0.9]
NEG = -1e9


def _bf(x):
  return x.float().to(torch.bfloat16).double()


def _err(got, ref):
  scale = float(ref.pow(2).mean().sqrt()) + 1e-8
  return float(((got.double().cpu() - ref).abs() / (scale + ref.abs())).max())


def _heads(x, H):
  b, t, c = x.shape
  return x.view(b, t, H, c // H).transpose(1, 2)


def _merge(x):
  b, h, t, d = x.shape
  return x.transpose(1, 2).reshape(b, t, h * d)


def _model(q, k, v, kb, H, scale, mask, keep, d_o=None, pos=None, window=0, back=0, emu=False):
  """float64 attention on host copies; emu = bf16 rounding at the kernel's rounding points."""
  rnd = _bf if emu else (lambda x: x)
  S = k.shape[1]
  Q, K, V = _heads(q, H), _heads(k, H), _heads(v, H)
  logits = scale * (Q @ K.transpose(-1, -2))
  bias = kb[:, None, None, :].float()
  if pos is not None:
    w = torch.clamp(pos.long() - back, min=0)[..., None]
    keys = torch.arange(S)[None, None, None, :]
    wm = torch.where((keys >= w) & (keys < w + window), 0.0, NEG).float()
    bias = torch.maximum(bias + wm, torch.tensor(NEG, dtype=torch.float32))
  x = (logits.float() + bias).double()          # the additive fp32 bias of the contract
  P = torch.softmax(x, -1)
  Pd = rnd(P * mask.double() / keep)
  out = {"p": P, "o": rnd(_merge(Pd @ V)), "labs": scale * (Q.abs() @ K.abs().transpose(-1, -2))}
  if d_o is not None:
    dO = _heads(d_o, H)
    g = (dO @ V.transpose(-1, -2)) * mask.double() / keep
    dS = rnd(P * (g - (P * g).sum(-1, keepdim=True)))
    out["dv"] = rnd(_merge(Pd.transpose(-1, -2) @ dO))
    out["dq"] = rnd(_merge(scale * (dS @ K)))
    out["dk"] = rnd(_merge(scale * (dS.transpose(-1, -2) @ Q)))
  return out


def _inputs(g, Tq, S, C, dev):
  qs = torch.randn(B, Tq, 3 * C, generator=g).to(torch.bfloat16).to(dev)
  ks = torch.randn(B, S, 2 * C + 8, generator=g).to(torch.bfloat16).to(dev)
  q, k, v = qs[:, :, C:2 * C], ks[:, :, :C], ks[:, :, C + 8:]
  counts = [S, 1, S - 3]
  kb = torch.zeros(B, S)
  for b in range(B):
    kb[b, counts[b]:] = NEG
  return (q, k, v), tuple(t.double().cpu().contiguous() for t in (q, k, v)), kb


def _check_p(got, ref, D, tag):
  tol = 2.0 * D * 2.0 ** -24 * float(ref["labs"].max()) + 1e-5
  diff = (got.double().cpu() - ref["p"]).abs()
  worst = float((diff / (tol * ref["p"] + 1e-9)).max())
  print("%s p err/bound %.3f (rtol %.2e)" % (tag, worst, tol))
  assert worst <= 1.0, (tag, worst)
  return worst


def _check_argmax(am, ref, tag):
  top = ref["p"].topk(2, -1) if ref["p"].shape[-1] > 1 else None
  sure = (top.values[..., 0] - top.values[..., 1]) > 1e-2
  assert bool(sure.any()), tag
  assert torch.equal(am.cpu().long()[sure], top.indices[..., 0][sure]), tag


def _run_case(capi, D, H, Tq, S, keep, bwd, seed, stats):
  dev = torch.device("cuda")
  C = H * D
  scale = float(D) ** -0.5
  g = torch.Generator().manual_seed(1000 * D + 100 * H + Tq + S + int(keep * 10))
  (q, k, v), (qf, kf, vf), kb = _inputs(g, Tq, S, C, dev)
  kbd = kb.to(dev)
  mask = torch.ones(B, H, Tq, S)
  if keep < 1.0:
    mask = capi.dropout_mask(seed, B * H * Tq * S, keep, dev).view(B, H, Tq, S).cpu().float()
  tag = "D%d H%d Tq%d S%d keep%.1f" % (D, H, Tq, S, keep)
  o, p, am = capi.attention_wide_fwd(q, k, v, kbd, H, scale, keep, seed, want_argmax=True)
  o2, p2, am2 = capi.attention_wide_fwd(q, k, v, kbd, H, scale, keep, seed, want_argmax=True)
  assert torch.equal(o, o2) and torch.equal(p, p2) and torch.equal(am, am2), tag
  d_of = None
  if bwd:
    d_o = torch.randn(B, Tq, C + 8, generator=g).to(torch.bfloat16).to(dev)[:, :, 8:]
    d_of = d_o.double().cpu().contiguous()
  ref = _model(qf, kf, vf, kb, H, scale, mask, keep, d_of)
  emu = _model(qf, kf, vf, kb, H, scale, mask, keep, d_of, emu=True)
  stats["p"] = max(stats.get("p", 0.0), _check_p(p, ref, D, tag))
  _check_argmax(am, ref, tag)
  names = ["o"]
  got = {"o": o}
  if bwd:
    bufs = [torch.full((B, T, C + 8), 7.0, dtype=torch.bfloat16, device=dev) for T in (Tq, S, S)]
    outs = capi.attention_wide_bwd(q, k, v, d_o, p, H, scale, keep, seed, *[t[:, :, :C] for t in bufs])
    again = capi.attention_wide_bwd(q, k, v, d_o, p, H, scale, keep, seed)
    for n, t, t2, buf in zip(("dq", "dk", "dv"), outs, again, bufs):
      assert torch.equal(t, t2), (tag, n)
      assert bool((buf[:, :, C:] == 7.0).all()), (tag, n)
      got[n] = t
      names.append(n)
  for n in names:
    e, bound = _err(got[n], ref[n]), 2.0 * _err(emu[n], ref[n])
    print("%s %s err %.3e bound %.3e" % (tag, n, e, bound))
    if e > stats.get(n, (0.0, 0.0))[0]:
      stats[n] = (e, bound)
    assert torch.isfinite(got[n].float()).all(), (tag, n)
    assert e <= bound, (tag, n, e, bound)


@pytest.mark.parametrize("H", [1, 2])
@pytest.mark.parametrize("D,bwd", [(32, True), (512, True), (64, False), (128, False), (256, False)])
def test_wide_attention_against_float64(D, bwd, H):
  from openseq2seq_amd import capi
  stats = {}
  seed = 77
  for Tq in TQS:
    for S in SS:
      for keep in KEEPS:
        seed += 1
        _run_case(capi, D, H, Tq, S, keep, bwd, seed, stats)
  print("WORST D%d H%d %s" % (D, H, stats))


@pytest.mark.parametrize("D", [32, 512])
def test_long_sources(D):
  """Both sides of S = 256, where the row pass goes from two rows per wave to one, and the limit S = 512 (the largest
  LDS request); forward and backward, with dropout."""
  from openseq2seq_amd import capi
  stats = {}
  for i, (Tq, S) in enumerate(((7, 256), (70, 264), (70, 512))):
    _run_case(capi, D, 1, Tq, S, 0.9, True, 300 + i, stats)
  print("WORST long D%d %s" % (D, stats))


@pytest.mark.parametrize("D", [32, 512])
def test_window_bias(D):
  """positions / window / back_step: inside the source, across the last real key, wholly past it, back_step 1 at 0."""
  from openseq2seq_amd import capi
  dev = torch.device("cuda")
  H, Tq, S = 2, 7, 72
  C = H * D
  scale = float(D) ** -0.5
  g = torch.Generator().manual_seed(5 + D)
  (q, k, v), (qf, kf, vf), kb = _inputs(g, Tq, S, C, dev)       # real keys: 72, 1, 69
  pos = torch.zeros(B, H, Tq, dtype=torch.int32)
  pos[0] = torch.tensor([[0, 20, 21, 40, 69, 70, 71], [1, 5, 9, 30, 31, 64, 68]], dtype=torch.int32)
  pos[1] = torch.tensor([[0, 1, 2, 10, 30, 69, 71], [0, 0, 1, 3, 4, 50, 70]], dtype=torch.int32)    # mostly past key 0
  pos[2] = torch.tensor([[0, 66, 67, 68, 69, 70, 71], [2, 64, 65, 66, 67, 68, 69]], dtype=torch.int32)
  ones = torch.ones(B, H, Tq, S)
  for window, back in ((3, 0), (5, 0), (4, 1)):
    tag = "D%d window %d back %d" % (D, window, back)
    o, p, am = capi.attention_wide_fwd(q, k, v, kb.to(dev), H, scale, positions=pos.to(dev), window=window,
                                       back_step=back, want_argmax=True)
    ref = _model(qf, kf, vf, kb, H, scale, ones, 1.0, pos=pos, window=window, back=back)
    emu = _model(qf, kf, vf, kb, H, scale, ones, 1.0, pos=pos, window=window, back=back, emu=True)
    assert torch.isfinite(p).all() and torch.isfinite(o.float()).all(), tag
    _check_p(p, ref, D, tag)
    _check_argmax(am, ref, tag)
    # a window wholly past the last real key: every key carries -1e9, the row is uniform, never NaN
    row = p[1, 0, 4].cpu()
    assert float((row - 1.0 / S).abs().max()) < 1e-6, tag
    if back == 1:     # position 0 with a step back stays at key 0
      assert float(p[0, 0, 0, :window].sum()) > 0.999, tag
    e, bound = _err(o, ref["o"]), 2.0 * _err(emu["o"], ref["o"])
    print("%s o err %.3e bound %.3e" % (tag, e, bound))
    assert e <= bound, (tag, e, bound)


def test_unsupported_shapes_are_errors():
  from openseq2seq_amd import _lib, capi
  from openseq2seq_amd.parts.centaur import attention as catt
  dev = torch.device("cuda")

  def call(D, S, H=1, Tq=4):
    q = torch.zeros(1, Tq, H * D, dtype=torch.bfloat16, device=dev)
    k = torch.zeros(1, S, H * D, dtype=torch.bfloat16, device=dev)
    return capi.attention_wide_fwd(q, k, k, torch.zeros(1, S, device=dev), H, 1.0)

  for D, S in ((48, 8), (1024, 8), (16, 8), (32, 520), (32, 12)):
    with pytest.raises(_lib.Os2sError, match=r"\(code -3\)"):
      call(D, S)
    q = torch.zeros(1, 4, D, dtype=torch.bfloat16, device=dev)
    k = torch.zeros(1, S, D, dtype=torch.bfloat16, device=dev)
    with pytest.raises(_lib.Os2sError, match=r"\(code -3\)"):
      capi.attention_wide_bwd(q, k, k, q, torch.zeros(1, 1, 4, S, device=dev), 1, 1.0)
    with pytest.raises(NotImplementedError):
      catt.check_shape(D, 1, S)
  call(32, 512)                      # the limits themselves are served
  assert catt.check_shape(512, 1, 184) == 512


def test_layer_records_gradients_once_per_input():
  """parts/centaur wide_attention on a Tape: the gradients of q, k and v are the kernel's, the alignments come back."""
  from openseq2seq_amd import capi
  from openseq2seq_amd.parts.centaur import padding_bias, wide_attention
  from openseq2seq_amd.parts.tape import Act, Tape
  dev = torch.device("cuda")
  g = torch.Generator().manual_seed(3)
  Tq, S, C = 9, 16, 64
  q, k, v = (Act(torch.randn(B, T, C, generator=g).to(torch.bfloat16).to(dev)) for T in (Tq, S, S))
  ids = torch.randint(1, 9, (B, S), generator=g)
  ids[1, 5:] = 0
  kb = padding_bias(ids.to(dev))
  assert kb.dtype is torch.float32 and float(kb[1, 5]) == NEG and float(kb[1, 4]) == 0.0
  tape = Tape()
  out, w, am = wide_attention(q, k, v, kb, 1, tape, keep_prob=0.9, seed=11)
  assert am is None and w.shape == (B, 1, Tq, S) and float(w[1, 0, :, 5:].max()) == 0.0
  out.grad = torch.randn(B, Tq, C, generator=g).to(torch.bfloat16).to(dev)
  d_o = out.grad
  tape.backward()
  dq, dk, dv = capi.attention_wide_bwd(q.data, k.data, v.data, d_o, w, 1, C ** -0.5, 0.9, 11)
  assert torch.equal(q.grad, dq) and torch.equal(k.grad, dk) and torch.equal(v.grad, dv)
