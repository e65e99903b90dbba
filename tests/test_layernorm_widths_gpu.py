"""LayerNorm rows of any width (the any-width kernels of csrc/layernorm.hip): layernorm_L2 and layernorm_L1
forward / backward at widths next to the tuned 512 / 1024 — below one 16-byte piece per lane (8, 32), no multiple of 64 pieces (72, 768), several
pieces per lane (2048) and the largest width (4096). N = 77 rows: three row blocks of the backward, the last one
partial. Residual-gradient input, dgamma / dbeta through the [num_parts, 2, D] partials. Bounds: those of
test_layernorm_fwd_bwd (tests/test_transformer_kernels_gpu.py) and test_layernorm_l1_fwd_bwd
(tests/test_transformer_norm_kernels_gpu.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

WIDTHS = [8, 32, 72, 128, 256, 768, 2048, 4096]
N = 77


def _close(got, ref, tol=2e-2):
  got = got.float().cpu()
  scale = float(ref.detach().pow(2).mean().sqrt()) + 1e-8
  torch.testing.assert_close(got, ref.detach(), rtol=tol, atol=tol * scale)


def _rel(a, b):
  a, b = a.double().cpu(), b.double().cpu()
  return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize("D", WIDTHS)
def test_layernorm_l2_widths(cuda, D):
  from openseq2seq_amd import capi
  from oracle import transformer as ot
  g = torch.Generator().manual_seed(1 + D)
  x = (torch.randn(N, D, generator=g) * 2 + 0.5).to(torch.bfloat16)
  gam, bet = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g) * 0.1
  dy = torch.randn(N, D, generator=g).to(torch.bfloat16)
  dres = torch.randn(N, D, generator=g).to(torch.bfloat16)
  y, mean, rstd = capi.layernorm_fwd(x.to(cuda), gam.to(cuda), bet.to(cuda))
  dgam, dbet = torch.zeros(D, device=cuda), torch.zeros(D, device=cuda)
  dx = capi.layernorm_bwd(dy.to(cuda), x.to(cuda), gam.to(cuda), mean, rstd, dres.to(cuda), dgam, dbet)
  torch.cuda.synchronize()
  xf, gf, bf = x.float().requires_grad_(True), gam.clone().requires_grad_(True), bet.clone().requires_grad_(True)
  ref = ot.layer_norm(xf, gf, bf)
  ref.backward(dy.float())
  _close(y, ref)
  _close(dx, xf.grad + dres.float())
  _close(dgam, gf.grad)
  _close(dbet, bf.grad)
  # without a residual gradient
  dx0 = capi.layernorm_bwd(dy.to(cuda), x.to(cuda), gam.to(cuda), mean, rstd, None, dgam, dbet)
  _close(dx0, xf.grad)


def _l1_rows(D, dev, seed):
  g = torch.Generator().manual_seed(seed)
  x = (torch.randn(N, D, generator=g) * 1.5 + 0.3).to(torch.bfloat16)
  x[0] = 0.75                                               # constant row: mean|c| = 0
  x[1] = torch.tensor([-1.0, 1.0, 0.0, 0.0] * (D // 4))     # ties at the mean: sign(c) = 0 there
  dy = torch.randn(N, D, generator=g).to(torch.bfloat16)
  dres = torch.randn(N, D, generator=g).to(torch.bfloat16)
  gamma = 1.0 + 0.1 * torch.randn(D, generator=g)
  beta = 0.1 * torch.randn(D, generator=g)
  return x.to(dev), dy.to(dev), dres.to(dev), gamma.to(dev), beta.to(dev)


@pytest.mark.parametrize("D", WIDTHS)
def test_layernorm_l1_widths(cuda, D):
  from openseq2seq_amd import capi
  eps = 1e-6
  x, dy, dres, gamma, beta = _l1_rows(D, cuda, 7 + N + D)
  y, mean, rinv = capi.layernorm_l1_fwd(x, gamma, beta, eps)
  dx, partial = capi.layernorm_l1_bwd(dy, x, gamma, mean, rinv, dres)
  dgamma = torch.zeros(D, device=cuda)
  dbeta = torch.zeros(D, device=cuda)
  scratch = torch.empty((2, D), device=cuda)
  capi.bn_bwd_finalize(partial, 1, 1, dgamma, dbeta, True, scratch[0], scratch[1])
  torch.cuda.synchronize()
  xr = x.float().cpu().requires_grad_(True)
  gr = gamma.cpu().clone().requires_grad_(True)
  br = beta.cpu().clone().requires_grad_(True)
  c = xr - xr.mean(-1, keepdim=True)
  yr = c / (c.abs().mean(-1, keepdim=True) + eps) * gr + br
  yr.backward(dy.float().cpu())
  assert _rel(y.float(), yr.detach()) < 1e-2
  assert torch.allclose(mean.cpu(), xr.detach().mean(-1), atol=1e-5)
  cd = c.detach()
  assert _rel(rinv, 1.0 / (cd.abs().mean(-1) + eps)) < 1e-5
  assert _rel(y[0].float(), beta) < 1e-2
  ref_dx = xr.grad + dres.float().cpu()
  assert _rel(dx[0].float(), ref_dx[0]) < 2e-2
  assert _rel(dx[1:].float(), ref_dx[1:]) < 2e-2
  assert _rel(dx[1].float(), ref_dx[1]) < 2e-2                # ties at the mean
  assert _rel(dgamma, gr.grad) < 1e-3
  assert _rel(dbeta, br.grad) < 1e-3


def _l1_ref(x, gamma, beta, eps):
  c = x - x.mean(-1, keepdim=True)
  return c / (c.abs().mean(-1, keepdim=True) + eps) * gamma + beta


@pytest.mark.parametrize("with_dres", [True, False])
@pytest.mark.parametrize("n", [1, 9, 32, 33])
@pytest.mark.parametrize("D", [512, 1024])
@pytest.mark.parametrize("kind", ["l2", "l1"])
def test_layernorm_tuned_row_blocks(cuda, kind, D, n, with_dres):
  """The tuned D = 512 / 1024 backward (csrc/layernorm.hip, one kernel template for both kinds) where its row
  prefetch meets an edge: fewer rows than the 8 waves of a workgroup (1), a partial second round of the waves (9),
  exactly one 32-row block (32) and one row past it (33); with a residual gradient and without one (the null
  buffer descriptor, whose loads all return zeros). Reference: torch autograd in fp64 from the bf16 inputs."""
  from openseq2seq_amd import capi
  eps = 1e-6
  g = torch.Generator().manual_seed(1000 * D + 10 * n + (kind == "l1"))
  x = (torch.randn(n, D, generator=g) * 1.5 + 0.3).to(torch.bfloat16)
  if kind == "l1" and n >= 2:
    x[0] = 0.75                                               # constant row: mean|c| = 0
    x[1] = torch.tensor([-1.0, 1.0, 0.0, 0.0] * (D // 4))     # ties at the mean: sign(c) = 0 there
  dy = torch.randn(n, D, generator=g).to(torch.bfloat16)
  dres = torch.randn(n, D, generator=g).to(torch.bfloat16)
  gamma = 1.0 + 0.1 * torch.randn(D, generator=g)
  beta = 0.1 * torch.randn(D, generator=g)
  xd, dyd, gd, bd = x.to(cuda), dy.to(cuda), gamma.to(cuda), beta.to(cuda)
  dresd = dres.to(cuda) if with_dres else None
  dgamma, dbeta = torch.zeros(D, device=cuda), torch.zeros(D, device=cuda)
  if kind == "l1":
    y, mean, rsave = capi.layernorm_l1_fwd(xd, gd, bd, eps)
    dx, partial = capi.layernorm_l1_bwd(dyd, xd, gd, mean, rsave, dresd)
    capi.colsum_finalize(partial, dgamma, dbeta)
  else:
    y, mean, rsave = capi.layernorm_fwd(xd, gd, bd, eps)
    dx = capi.layernorm_bwd(dyd, xd, gd, mean, rsave, dresd, dgamma, dbeta)
  torch.cuda.synchronize()
  xr = x.double().requires_grad_(True)
  gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
  if kind == "l1":
    yr = _l1_ref(xr, gr, br, eps)
  else:
    yr = torch.nn.functional.layer_norm(xr, (D,), gr, br, eps)
  yr.backward(dy.double())
  ref_dx = xr.grad + (dres.double() if with_dres else 0.0)
  if kind == "l2":
    _close(y, yr.float())
    _close(dx, ref_dx.float())
    _close(dgamma, gr.grad.float())
    _close(dbeta, br.grad.float())
    return
  assert _rel(y.float(), yr.detach()) < 1e-2
  assert torch.allclose(mean.cpu().double(), xr.detach().mean(-1), atol=1e-5)
  c = xr.detach() - xr.detach().mean(-1, keepdim=True)
  assert _rel(rsave, 1.0 / (c.abs().mean(-1) + eps)) < 1e-5
  split = 2 if n >= 2 else 0                                  # the two special rows on their own, as above
  for rows in [slice(i, i + 1) for i in range(split)] + [slice(split, n)]:
    assert _rel(dx[rows].float(), ref_dx[rows]) < 2e-2, rows
  assert _rel(dgamma, gr.grad) < 1e-3
  assert _rel(dbeta, br.grad) < 1e-3
