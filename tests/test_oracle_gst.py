"""CPU cross-checks that tie the float64 references of tests/_gst_ref.py to the TF-semantics oracles, so the
kernel-level GPU tests (test_gst_kernels_gpu.py, test_conv2d_toeplitz_gpu.py) can trust them:
oracle.gst.gru_cell_tf vs the direct per-step recurrence on precomputed input projections,
oracle.gst.token_attention vs token_attention_ref, the Toeplitz expansion contracted with an input vs
oracle.ds2.conv2d_tf, and the reduction as the exact adjoint of the expansion. Everything runs in float64 and
must agree to 1e-12."""
import pytest
import torch

import _gst_ref as R
from oracle import ds2 as ods, gst as ogst

F64 = torch.float64
TOL = 1e-12


def _maxdiff(a, b):
  assert a.shape == b.shape, (a.shape, b.shape)
  return float((a - b).abs().max())


@pytest.mark.parametrize("B,T,In,H", [(5, 6, 7, 9), (3, 4, 5, 16)])
def test_gru_cell_tf_equals_per_step_recurrence(B, T, In, H):
  g = torch.Generator().manual_seed(B * 100 + T)
  x = torch.randn(B, T, In, generator=g, dtype=F64)
  wg = torch.randn(In + H, 2 * H, generator=g, dtype=F64) * (In + H) ** -0.5
  wc = torch.randn(In + H, H, generator=g, dtype=F64) * (In + H) ** -0.5
  bg = torch.randn(2 * H, generator=g, dtype=F64)
  bc = torch.randn(H, generator=g, dtype=F64)
  dh = torch.randn(B, H, generator=g, dtype=F64)
  lens = torch.tensor([T, 0, 1, T - 1, 2][:B])                       # ragged, with 0 and T
  xl = x.clone().requires_grad_(True)
  want = ogst.gru_cell_tf(xl, lens, wg, bg, wc, bc)
  got = R.gru_tf_ref(x @ wg[:In] + bg, x @ wc[:In] + bc, wg[In:], wc[In:], lens, dh_final=dh)
  assert _maxdiff(got["h_final"], want.detach()) <= TOL
  assert torch.equal(got["h_final"], got["h_seq"][:, T])
  assert torch.equal(got["h_final"][1], torch.zeros(H, dtype=F64))   # len 0: the zero state comes through
  # the gradients of the projections, pulled back onto x, are the oracle's gradient of x
  (dx,) = torch.autograd.grad(want, xl, dh)
  mine = got["dgxg"] @ wg[:In].t() + got["dgxc"] @ wc[:In].t()
  assert _maxdiff(mine, dx) <= TOL
  for b in range(B):
    n = int(lens[b])
    assert not got["dgxg"][b, n:].any() and not got["dgxc"][b, n:].any()
    assert not got["r"][b, n:].any() and not got["c"][b, n:].any() and not got["hprev"][b, n:].any()
    assert not got["rh"][b, n:].any() and bool((got["u"][b, n:] == 1).all())


def test_gru_ref_clamps_lengths_and_defaults_to_full():
  g = torch.Generator().manual_seed(4)
  B, T, H = 3, 5, 6
  gxg = torch.randn(B, T, 2 * H, generator=g, dtype=F64)
  gxc = torch.randn(B, T, H, generator=g, dtype=F64)
  wgh = torch.randn(H, 2 * H, generator=g, dtype=F64) * H ** -0.5
  wch = torch.randn(H, H, generator=g, dtype=F64) * H ** -0.5
  a = R.gru_tf_ref(gxg, gxc, wgh, wch, torch.tensor([T + 3, -2, T]))
  b = R.gru_tf_ref(gxg, gxc, wgh, wch, torch.tensor([T, 0, T]))
  c = R.gru_tf_ref(gxg, gxc, wgh, wch, None)
  for k in a:
    assert torch.equal(a[k], b[k]), k
  assert torch.equal(a["h_seq"][0], c["h_seq"][0]) and torch.equal(a["h_seq"][2], c["h_seq"][2])
  assert not torch.equal(a["h_seq"][1], c["h_seq"][1])


@pytest.mark.parametrize("B,heads,N", [(3, 2, 10), (1, 1, 1), (4, 3, 64)])
def test_token_attention_equals_oracle(B, heads, N):
  g = torch.Generator().manual_seed(B + 10 * heads + N)
  D = heads * 64
  q = torch.randn(B, D, generator=g, dtype=F64)
  k = torch.randn(N, D, generator=g, dtype=F64)
  v = torch.randn(N, D, generator=g, dtype=F64)
  att_v = torch.randn(64, generator=g, dtype=F64)
  dout = torch.randn(B, D, generator=g, dtype=F64)
  eye, zero = torch.eye(D, dtype=F64), torch.zeros(D, D, dtype=F64)
  leaves = [t.clone().requires_grad_(True) for t in (q, k, v, att_v)]
  ql, kl, vl, al = leaves
  # the oracle projects one token matrix to keys and values: tokens = [k | v] with selector kernels
  want = ogst.token_attention(ql, torch.cat([kl, vl], 1), eye, torch.cat([eye, zero], 0),
                              torch.cat([zero, eye], 0), eye, al, heads)
  got = R.token_attention_ref(q, k, v, att_v, heads, dout=dout)
  assert _maxdiff(got["out"], want.detach()) <= TOL
  assert float((got["w"].sum(-1) - 1).abs().max()) <= TOL
  grads = torch.autograd.grad(want, leaves, dout)
  for name, gr in zip(("dq", "dk", "dv", "datt_v"), grads):
    assert _maxdiff(got[name], gr) <= TOL, name


def _time_geometry(T, KT, sT, padding):
  if padding == "SAME":
    To = -(-T // sT)
    total = max((To - 1) * sT + KT - T, 0)
    return To, total // 2, total - total // 2
  return (T - KT) // sT + 1, 0, 0


@pytest.mark.parametrize("sT", [1, 2])
@pytest.mark.parametrize("KT,KF,Cin,Cout,Fi,sF,padding", R.TOEPLITZ_CASES)
def test_toeplitz_expansion_is_conv2d_tf(KT, KF, Cin, Cout, Fi, sF, padding, sT):
  g = torch.Generator().manual_seed(KT * 1000 + KF * 10 + Fi)
  B, T = 2, 13
  Fo, padF = R.toeplitz_geometry(Fi, KF, sF, padding)
  assert (Fi * Cin) % 8 == 0 and (Fo * Cout) % 8 == 0
  w = torch.randn(KT, KF, Cin, Cout, generator=g, dtype=F64)
  x = torch.randn(B, T, Fi * Cin, generator=g, dtype=F64)
  want = ods.conv2d_tf(x.view(B, T, Fi, Cin), w, [sT, sF], padding)  # [B, To, Fo, Cout]
  wexp = R.toeplitz_expand_ref(w, Fi, Fo, sF, padF)
  To, pl, pr = _time_geometry(T, KT, sT, padding)
  xp = torch.nn.functional.pad(x, (0, 0, pl, pr))
  got = torch.zeros(B, To, Fo * Cout, dtype=F64)
  for kt in range(KT):
    got += torch.einsum("btj,oj->bto", xp[:, kt:kt + (To - 1) * sT + 1:sT], wexp[kt])
  assert tuple(want.shape) == (B, To, Fo, Cout)
  assert _maxdiff(got, want.reshape(B, To, Fo * Cout)) <= TOL


@pytest.mark.parametrize("KT,KF,Cin,Cout,Fi,sF,padding", R.TOEPLITZ_CASES)
def test_toeplitz_reduce_is_adjoint_of_expand(KT, KF, Cin, Cout, Fi, sF, padding):
  g = torch.Generator().manual_seed(KT + KF + Fi)
  Fo, padF = R.toeplitz_geometry(Fi, KF, sF, padding)
  w = torch.randn(KT, KF, Cin, Cout, generator=g, dtype=F64)
  G = torch.randn(KT, Fo * Cout, Fi * Cin, generator=g, dtype=F64)
  lhs = float((R.toeplitz_expand_ref(w, Fi, Fo, sF, padF) * G).sum())
  rhs = float((w * R.toeplitz_reduce_ref(G, KF, Cin, Cout, Fi, Fo, sF, padF)).sum())
  assert abs(lhs - rhs) <= TOL * max(1.0, abs(lhs))
  # the band is where the expansion of an all-ones kernel is non-zero; everything else is +0
  band = R.toeplitz_expand_ref(torch.ones_like(w), Fi, Fo, sF, padF)
  assert int(band.sum()) == KT * Cin * Cout * sum(
      1 for fo in range(Fo) for fi in range(Fi) if 0 <= fi - fo * sF + padF < KF)
