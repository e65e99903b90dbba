"""The norm_params kernels of the Transformer (csrc/layernorm.hip, csrc/transformer_norm.hip) against fp32 torch autograd:
layernorm_L1 forward / backward (parts/transformer/common.py:69-80) and the token BatchNorm over packed [N, D]
rows (common.py:11-38: training statistics, moving-statistics update, eval apply, backward with and without
center_scale). Bounds are those of test_layernorm_fwd_bwd (tests/test_transformer_e2e_gpu.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rel(a, b):
  a, b = a.double().cpu(), b.double().cpu()
  return float((a - b).norm() / (b.norm() + 1e-30))


def _rows(N, D, dev, seed):
  g = torch.Generator().manual_seed(seed)
  x = (torch.randn(N, D, generator=g) * 1.5 + 0.3).to(torch.bfloat16)
  x[0] = 0.75                                               # constant row: mean|c| = 0
  if N > 1:
    x[1] = torch.tensor([-1.0, 1.0, 0.0, 0.0] * (D // 4))   # ties at the mean: sign(c) = 0 there
  dy = torch.randn(N, D, generator=g).to(torch.bfloat16)
  dres = torch.randn(N, D, generator=g).to(torch.bfloat16)
  gamma = 1.0 + 0.1 * torch.randn(D, generator=g)
  beta = 0.1 * torch.randn(D, generator=g)
  return x.to(dev), dy.to(dev), dres.to(dev), gamma.to(dev), beta.to(dev)


def _l1_ref(x, gamma, beta, eps):
  c = x - x.mean(-1, keepdim=True)
  a = c.abs().mean(-1, keepdim=True)
  return c / (a + eps) * gamma + beta


@pytest.mark.parametrize("D", [512, 1024])
@pytest.mark.parametrize("N", [77, 16384])
def test_layernorm_l1_fwd_bwd(cuda, N, D):
  from openseq2seq_amd import capi
  eps = 1e-6
  x, dy, dres, gamma, beta = _rows(N, D, cuda, 7 + N + D)
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
  yr = _l1_ref(xr, gr, br, eps)
  yr.backward(dy.float().cpu())
  assert _rel(y.float(), yr.detach()) < 1e-2
  assert torch.allclose(mean.cpu(), xr.detach().mean(-1), atol=1e-5)
  c = xr.detach() - xr.detach().mean(-1, keepdim=True)
  assert _rel(rinv, 1.0 / (c.abs().mean(-1) + eps)) < 1e-5
  # the constant row: y = beta exactly up to bf16 rounding; its gradient is g r - mean(g r) with r = 1 / eps
  assert _rel(y[0].float(), beta) < 1e-2
  ref_dx = xr.grad + dres.float().cpu()
  # the constant row's gradient is 1e6 times the others': held on its own, the rest together
  assert _rel(dx[0].float(), ref_dx[0]) < 2e-2
  assert _rel(dx[1:].float(), ref_dx[1:]) < 2e-2
  assert _rel(dx[1].float(), ref_dx[1]) < 2e-2                # ties at the mean
  assert _rel(dgamma, gr.grad) < 1e-3
  assert _rel(dbeta, br.grad) < 1e-3


def _bn_ref(x, gamma, beta, eps):
  m = x.mean(0)
  v = x.var(0, unbiased=False)
  return (x - m) / torch.sqrt(v + eps) * gamma + beta


@pytest.mark.parametrize("center_scale", [True, False])
@pytest.mark.parametrize("D,N", [(512, 77), (1024, 16384), (512, 3)])
def test_token_batchnorm_train_fwd_bwd(cuda, D, N, center_scale):
  from openseq2seq_amd import capi
  eps, momentum = 1e-5, 0.95
  x, dy, dres, gamma, beta = _rows(N, D, cuda, 100 + N + D)
  if not center_scale:
    gamma = beta = None
  mm0 = 0.1 * torch.randn(D, device=cuda)
  mv0 = 1.0 + torch.rand(D, device=cuda)
  mm, mv = mm0.clone(), mv0.clone()
  vec = torch.empty((4, D), device=cuda)
  capi.bn_finalize(capi.bn_stats(x), N, gamma, beta, eps, momentum, True, mm, mv, vec[2], vec[3], vec[0], vec[1])
  y = capi.token_bn_apply(x, vec[0], vec[1])
  partial = capi.token_bn_bwd_reduce(dy, x, vec[2], vec[3])
  dgamma = torch.zeros(D, device=cuda) if center_scale else None
  dbeta = torch.zeros(D, device=cuda) if center_scale else None
  c = torch.empty((2, D), device=cuda)
  capi.bn_bwd_finalize(partial, 1, N, dgamma, dbeta, True, c[0], c[1])
  dx = capi.token_bn_bwd_apply(dy, x, gamma, vec[2], vec[3], c[0], c[1], dres)
  torch.cuda.synchronize()
  xr = x.float().cpu().requires_grad_(True)
  gr = (gamma.cpu() if center_scale else torch.ones(D)).clone().requires_grad_(True)
  br = (beta.cpu() if center_scale else torch.zeros(D)).clone().requires_grad_(True)
  yr = _bn_ref(xr, gr, br, eps)
  yr.backward(dy.float().cpu())
  assert _rel(y.float(), yr.detach()) < 1e-2
  assert _rel(dx.float(), xr.grad + dres.float().cpu()) < 2e-2
  if center_scale:
    assert _rel(dgamma, gr.grad) < 1e-3
    assert _rel(dbeta, br.grad) < 1e-3
  # moving statistics: TF fused-BN conventions, count = N (Bessel-corrected variance in the moving average)
  xd = xr.detach().double()
  bm, bv = xd.mean(0), xd.var(0, unbiased=True)
  assert _rel(mm, mm0.double().cpu() * momentum + bm * (1 - momentum)) < 1e-5
  assert _rel(mv, mv0.double().cpu() * momentum + bv * (1 - momentum)) < 1e-5


@pytest.mark.parametrize("center_scale", [True, False])
@pytest.mark.parametrize("N", [12, 4096])
def test_token_batchnorm_eval_apply(cuda, N, center_scale):
  """eval / infer: the per-row affine map of the moving statistics (also the beam-search step, [B * beam, D])."""
  from openseq2seq_amd import capi
  D, eps = 512, 1e-4
  x, _, _, gamma, beta = _rows(N, D, cuda, 5 + N)
  if not center_scale:
    gamma = beta = None
  mm = 0.2 * torch.randn(D, device=cuda)
  mv = 0.5 + torch.rand(D, device=cuda)
  mm_before, mv_before = mm.clone(), mv.clone()
  sc, sh = torch.empty(D, device=cuda), torch.empty(D, device=cuda)
  capi.bn_finalize(None, N, gamma, beta, eps, 0.95, False, mm, mv, None, None, sc, sh)
  y = capi.token_bn_apply(x, sc, sh)
  torch.cuda.synchronize()
  g = gamma.cpu() if center_scale else torch.ones(D)
  b = beta.cpu() if center_scale else torch.zeros(D)
  ref = (x.float().cpu() - mm.cpu()) / torch.sqrt(mv.cpu() + eps) * g + b
  assert _rel(y.float(), ref) < 1e-2
  assert torch.equal(mm, mm_before) and torch.equal(mv, mv_before)
