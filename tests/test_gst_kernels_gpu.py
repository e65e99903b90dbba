"""Kernel-level accuracy of csrc/gst.hip against the float64 references of tests/_gst_ref.py:
gru_tf_fwd_kernel / gru_tf_bwd_kernel (tf GRUCell under dynamic_rnn: both candidate slots cn[0] / cn[1], the
length edges 0, 1, T-1, T, beyond T, negative and None) and gst_attn_fwd_kernel / gst_attn_bwd_kernel (N = 1 and
N = 64, the limits of the unrolled 64-entry arrays; the accumulate semantics of dk, dv and datt_v in both launch
geometries). The kernels keep state, saved activations and softmax in fp32, so every output is either an fp32
value a float64 reference predicts to ~1e-6 or a bf16 store of one: see close32 / close16 for the two bounds."""
import functools

import pytest
import torch

import _gst_ref as R

pytestmark = pytest.mark.gpu

# fp32 bound, relative to max|ref| of the tensor: see close32. It must stay <= 1e-4; a measurement that needs more
# would be a finding about the kernel, not a reason to widen it.
TOL32_MEASURED = 1.22e-6
TOL32 = 8 * TOL32_MEASURED        # 9.76e-6
assert TOL32 <= 1e-4

H_MAX, N_MAX = 512, 64      # OS2S_REQUIRE limits of the launchers; the cases stay inside them


def _ratio(name, got, ref):
  err = float((got - ref).abs().max())
  scale = float(ref.abs().max())
  print("ratio32 %-28s err %.3e  max|ref| %.3e  ratio %.3e" % (name, err, scale, err / scale if scale else 0.0))
  return err, scale


def close32(name, got, ref, prefill=None):
  """fp32 output: |got - ref| <= TOL32 * max|ref| over the WHOLE tensor (no element masked out). The kernels hold
  these values in fp32 end to end, so the float64 reference of the same bf16 / fp32 inputs predicts them up to the
  device's __expf / tanhf and the fp32 summation order; the fp32 restatement on the CPU differs from float64 by
  <= 5e-7 * max|ref|. MEASURED on an MI355X over every fp32 comparison of this file (GRU forward, attention forward,
  attention backward in both launch geometries): the largest max|got - ref| / max|ref| was 1.216e-6 (c_seq of the
  H = 512 GRU; attention 8.2e-7: dk at N = 64, datt_v after B * heads = 264 adds). TOL32 = 8x that = 9.76e-6: three
  bits of margin for other seeds, the order of the atomic adds and compiler reordering. With `prefill` (got = result - prefill of an accumulating output) the absolute floor rises to
  2**-22 * max|prefill|: each add rounds at the magnitude of the running sum, not of the contribution."""
  got, ref = got.detach().cpu().to(torch.float64), ref.to(torch.float64)
  assert got.shape == ref.shape, (name, got.shape, ref.shape)
  assert bool(torch.isfinite(got).all()), name
  err, scale = _ratio(name, got, ref)
  bound = TOL32 * scale
  if prefill is not None:
    bound = max(bound, 2.0 ** -22 * float(prefill.abs().max()))
  assert err <= bound, (name, err, bound)


def close16(name, got, ref):
  """bf16 output: |got - ref| <= 2**-8 * |ref| + TOL32 * max|ref| per element, whole tensor. 2**-8 * |ref| is one
  bf16 ulp: round-to-nearest-even gives half an ulp and the fp32 error may move a value across a rounding
  boundary."""
  assert got.dtype == torch.bfloat16, name
  got, ref = got.detach().cpu().to(torch.float64), ref.to(torch.float64)
  assert got.shape == ref.shape, (name, got.shape, ref.shape)
  assert bool(torch.isfinite(got).all()), name
  excess = (got - ref).abs() - (2.0 ** -8 * ref.abs() + TOL32 * float(ref.abs().max()))
  worst = float(excess.max())
  print("bound16 %-28s worst excess %.3e (max|ref| %.3e)" % (name, worst, float(ref.abs().max())))
  assert worst <= 0, (name, worst, int((excess > 0).sum()))


def _bits(t):
  t = t.detach().cpu()
  return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def bits_equal(a, b):
  return torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ GRUCell
GRU_CASES = [(4, 9, 32),       # baseline
             (3, 16, 128),     # the style encoder's real size
             (5, 7, 300),      # second candidate slot, partly filled
             (2, 5, 512)]      # second candidate slot full, at the H limit
# "ragged" holds T, 0, 1 and T-1. A batch of fewer than four samples cannot hold all four at once, so the vector is
# run in two rotations whose union does (B >= 4: each holds all four).
LEN_KINDS = ["ragged", "ragged_rot", "clamp", "none"]


def _lens(kind, B, T):
  vals = [T, 0, 1, T - 1]
  if kind == "ragged":
    return [vals[i % 4] for i in range(B)]
  if kind == "ragged_rot":
    return [vals[(i + 2) % 4] for i in range(B)]
  if kind == "clamp":
    return ([T + 3, -2] + [T // 2, T, 2])[:B]      # one beyond T, one negative
  return None


@functools.lru_cache(maxsize=None)
def _gru_case(B, T, H, kind):
  """Inputs and the float64 reference of one case, computed once and shared (read-only) by the tests."""
  assert 1 <= H <= H_MAX
  g = torch.Generator().manual_seed(1000 * B + 10 * T + H)
  gxg = torch.randn(B, T, 2 * H, generator=g).to(torch.bfloat16)
  gxc = torch.randn(B, T, H, generator=g).to(torch.bfloat16)
  wgh = torch.randn(H, 2 * H, generator=g) * H ** -0.5
  wch = torch.randn(H, H, generator=g) * H ** -0.5
  dh = torch.randn(B, H, generator=g)
  lens = _lens(kind, B, T)
  lens_t = None if lens is None else torch.tensor(lens, dtype=torch.int32)
  ref = R.gru_tf_ref(gxg, gxc, wgh, wch, lens_t, dh_final=dh)
  eff = [T] * B if lens is None else [min(max(n, 0), T) for n in lens]
  return dict(gxg=gxg, gxc=gxc, wgh=wgh, wch=wch, dh=dh, lens=lens_t, eff=eff, ref=ref)


def _gru_fwd(capi, cuda, c):
  lens = None if c["lens"] is None else c["lens"].to(cuda)
  sv = capi.gru_tf_fwd(c["gxg"].to(cuda), c["gxc"].to(cuda), c["wgh"].to(cuda), c["wch"].to(cuda), lens)
  torch.cuda.synchronize()
  return sv, lens


def _dead_mask(eff, T):
  return torch.tensor([[t >= n for t in range(T)] for n in eff])       # [B, T]


@pytest.mark.parametrize("kind", LEN_KINDS)
@pytest.mark.parametrize("B,T,H", GRU_CASES)
def test_gru_tf_fwd(cuda, B, T, H, kind):
  from openseq2seq_amd import capi
  c = _gru_case(B, T, H, kind)
  ref = c["ref"]
  sv, _ = _gru_fwd(capi, cuda, c)
  tag = "gru_fwd[%d,%d,%d,%s]." % (B, T, H, kind)
  close32(tag + "h_seq", sv["h_seq"], ref["h_seq"])
  close32(tag + "r_seq", sv["r_seq"], ref["r"])
  close32(tag + "u_seq", sv["u_seq"], ref["u"])
  close32(tag + "c_seq", sv["c_seq"], ref["c"])
  close32(tag + "h_final", sv["h_final"], ref["h_final"])
  close16(tag + "hprev16", sv["hprev16"], ref["hprev"])
  close16(tag + "rh16", sv["rh16"], ref["rh"])
  h_seq = sv["h_seq"].cpu()
  assert bits_equal(h_seq[:, 0], torch.zeros(B, H))                    # +0, not just == 0
  assert bits_equal(sv["h_final"], h_seq[:, T])
  dead = _dead_mask(c["eff"], T)
  if kind != "none":
    assert bool(dead.any())
  zero32, zero16 = torch.zeros(int(dead.sum()), H), torch.zeros(int(dead.sum()), H, dtype=torch.bfloat16)
  assert bits_equal(sv["r_seq"].cpu()[dead], zero32)
  assert bits_equal(sv["u_seq"].cpu()[dead], torch.ones(int(dead.sum()), H))
  assert bits_equal(sv["c_seq"].cpu()[dead], zero32)
  assert bits_equal(sv["hprev16"].cpu()[dead], zero16)
  assert bits_equal(sv["rh16"].cpu()[dead], zero16)
  assert bits_equal(h_seq[:, 1:][dead], h_seq[:, :-1][dead])            # state carried through t >= len
  again, _ = _gru_fwd(capi, cuda, c)
  for k in sv:
    assert bits_equal(sv[k], again[k]), k


@pytest.mark.parametrize("kind", LEN_KINDS)
@pytest.mark.parametrize("B,T,H", GRU_CASES)
def test_gru_tf_bwd(cuda, B, T, H, kind):
  """The backward kernel is fed the forward kernel's own saved tensors, as the layer does. capi.gru_tf_bwd
  allocates dgxg / dgxc itself (torch.empty), so they cannot be pre-filled with a sentinel: an unwritten row
  shows only through the exact-zero check and the comparison of the full tensors."""
  from openseq2seq_amd import capi
  c = _gru_case(B, T, H, kind)
  ref = c["ref"]
  sv, lens = _gru_fwd(capi, cuda, c)

  def run():
    out = capi.gru_tf_bwd(c["dh"].to(cuda), c["wgh"].t().contiguous().to(cuda),
                          c["wch"].t().contiguous().to(cuda), lens, sv)
    torch.cuda.synchronize()
    return out
  dgxg, dgxc = run()
  tag = "gru_bwd[%d,%d,%d,%s]." % (B, T, H, kind)
  assert tuple(dgxg.shape) == (B, T, 2 * H) and tuple(dgxc.shape) == (B, T, H)
  close16(tag + "dgxg", dgxg, ref["dgxg"])
  close16(tag + "dgxc", dgxc, ref["dgxc"])
  dead = _dead_mask(c["eff"], T)
  n = int(dead.sum())
  assert bits_equal(dgxg.cpu()[dead], torch.zeros(n, 2 * H, dtype=torch.bfloat16))
  assert bits_equal(dgxc.cpu()[dead], torch.zeros(n, H, dtype=torch.bfloat16))
  for b, m in enumerate(c["eff"]):
    if m == 0:                                                          # the whole sample
      assert not dgxg[b].any() and not dgxc[b].any()
    else:
      assert bool(dgxc[b, :m].any())
  a2, b2 = run()
  assert bits_equal(dgxg, a2) and bits_equal(dgxc, b2)


# ------------------------------------------------------------------------------------------------ token attention
ATT_CASES = [(3, 2, 10), (1, 1, 1), (5, 3, 64), (33, 8, 32)]


@functools.lru_cache(maxsize=None)
def _att_case(B, heads, N):
  assert 1 <= N <= N_MAX
  g = torch.Generator().manual_seed(100 * B + 10 * heads + N)
  D = heads * 64
  bf = torch.bfloat16
  q = torch.randn(B, D, generator=g).to(bf)
  k = torch.randn(N, D, generator=g).to(bf)
  v = torch.randn(N, D, generator=g).to(bf)
  att_v = torch.randn(64, generator=g)
  dout = torch.randn(B, D, generator=g).to(bf)
  pre = dict(dk=torch.randn(N, D, generator=g), dv=torch.randn(N, D, generator=g),
             datt_v=torch.randn(64, generator=g))
  assert all(bool((p != 0).all()) for p in pre.values())
  ref = R.token_attention_ref(q, k, v, att_v, heads, dout=dout)
  return dict(q=q, k=k, v=v, att_v=att_v, dout=dout, pre=pre, ref=ref)


@pytest.fixture
def det(cuda):
  from openseq2seq_amd import capi
  before = capi.deterministic()
  try:
    yield capi
  finally:
    capi.set_deterministic(before)


@pytest.mark.parametrize("B,heads,N", ATT_CASES)
def test_gst_attention_fwd(cuda, B, heads, N):
  from openseq2seq_amd import capi
  c = _att_case(B, heads, N)
  ref = c["ref"]
  out, w = capi.gst_attention_fwd(c["q"].to(cuda), c["k"].to(cuda), c["v"].to(cuda), c["att_v"].to(cuda), heads)
  torch.cuda.synchronize()
  tag = "att_fwd[%d,%d,%d]." % (B, heads, N)
  assert tuple(w.shape) == (B, heads, N) and w.dtype == torch.float32
  close32(tag + "w", w, ref["w"])
  assert float((w.cpu().double().sum(-1) - 1).abs().max()) <= 1e-6
  close16(tag + "out", out, ref["out"])
  if N == 1:
    assert bits_equal(w, torch.ones(B, heads, 1))
    assert bits_equal(out, c["v"].expand(B, -1).contiguous())


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("B,heads,N", ATT_CASES)
def test_gst_attention_bwd(det, cuda, B, heads, N, deterministic):
  """dk, dv and datt_v ACCUMULATE (StyleEncoder hands the live parameter gradient att_v.grad straight in): they
  are pre-filled with non-zero values and got - prefill is compared."""
  capi = det
  capi.set_deterministic(deterministic)
  c = _att_case(B, heads, N)
  ref, pre = c["ref"], c["pre"]
  q, k, v, att_v = (c[n].to(cuda) for n in ("q", "k", "v", "att_v"))
  _, w = capi.gst_attention_fwd(q, k, v, att_v, heads)
  acc = {n: p.clone().to(cuda) for n, p in pre.items()}
  dq = capi.gst_attention_bwd(c["dout"].to(cuda), q, k, v, att_v, w, heads, acc["dk"], acc["dv"], acc["datt_v"])
  torch.cuda.synchronize()
  tag = "att_bwd[%d,%d,%d,%s]." % (B, heads, N, "det" if deterministic else "atomic")
  for n in ("dk", "dv", "datt_v"):
    got = acc[n].cpu().double() - pre[n].double()
    close32(tag + n, got, ref[n], prefill=pre[n])
  close16(tag + "dq", dq, ref["dq"])
