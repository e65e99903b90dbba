"""GPU tests of the optimizer tail: the per-chunk sums of w^2 the update leaves for the next step's statistics pass
(LARC) against the pass that reads every tensor's weights — bit for bit, through a skipped step and through every
kind of write into the weights behind the optimizer's back —, the checking mode on two small models, and the masked
zero fill of the gradient buffer.

The trajectories are compared on the RAW flat buffers (`store._master`, ...): reading the public `master` attribute
marks the weights as possibly written, which would switch the cache off in the run under test."""
import copy
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import optim as oopt  # noqa: E402

# the chunk is 4096 elements: one element, one short of / exactly / one past a chunk, several chunks and a tail
VECTORS = [(1,), (4095,), (4096,), (4097,), (3 * 4096 + 5,)]
CONVS = [(3, 72, 40), (1, 8, 200)]
SHAPES = VECTORS + CONVS
NOVOGRAD = dict(beta1=0.95, beta2=0.98, epsilon=1e-8, weight_decay=0.001, grad_averaging=False)
POLY = dict(learning_rate=0.02, min_lr=1e-5, power=2.0, decay_steps=1000)
LARC = dict(larc_eta=0.001)


def _store(cuda, need_m2=False):
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  rng = np.random.RandomState(0)
  store, ws = FlatParams(cuda), []
  for i, s in enumerate(SHAPES):
    ws.append((rng.randn(*s) * 0.1).astype(np.float32))
    store.add("v%d" % i, s, ws[-1], kind="conv" if len(s) == 3 else "vector")
  store.finalize(need_m2=need_m2)
  return store, ws, rng


def _snapshot(store, op):
  torch.cuda.synchronize()
  st = op.read_state()
  return dict(master=store._master.clone(), m1=store._m1.clone(), w16=store._w16.clone(), wt16=store._wt16.clone(),
              wnorm2=store.t_wnorm2.clone(), scale=st["loss_scale"], skip=st["skip"], step=st["global_step"])


def _equal(a, b, what):
  for k in ("master", "m1", "w16", "wt16", "wnorm2"):
    assert torch.equal(a[k], b[k]), (what, k)
  assert (a["scale"], a["skip"], a["step"]) == (b["scale"], b["skip"], b["step"]), (what, a, b)


def _trajectory(cuda, monkeypatch, cached, between=None, nsteps=6, inf_step=2, check=False, ref=False):
  """NovoGrad with the Jasper parameters, LARC, Backoff scaling; an Inf gradient on step `inf_step`.
  between(step, store): writes into the weights after step `step`. Returns the snapshots (and the oracle)."""
  from openseq2seq_amd.optimizers import flat_params, lr_policies
  from openseq2seq_amd.optimizers.novograd import NovoGrad
  from openseq2seq_amd.optimizers.optimizers import optimize_loss
  monkeypatch.setattr(flat_params, "CACHED_WNORM", cached)
  monkeypatch.setattr(flat_params, "CHECK_WNORM", check)
  store, ws, rng = _store(cuda)
  op = optimize_loss(store, NovoGrad, NOVOGRAD, lr_policies.poly_decay, POLY, larc_params=LARC, loss_scaling="Backoff")
  oracle = oopt.RefOptimizer(ws, optimizer="NovoGrad", opt_params=NOVOGRAD, lr_fn=lambda s: oopt.poly_decay(s, **POLY),
                             larc_params=LARC, clip_gradients=None, scaler=oopt.BackoffScaler(), l2=None,
                             world_size=1) if ref else None
  snaps, cached_tensors = [], []
  for step in range(nsteps):
    scale = float(op.read_state()["loss_scale"])
    grads = [(rng.randn(*s) * 0.01).astype(np.float32) * scale for s in SHAPES]
    if step == inf_step:
      grads[4][17] = np.inf
    for p, g in zip(store.params, grads):
      p.grad.copy_(torch.from_numpy(g))
    cached_tensors.append(sum(not p.need_w for p in store.params))
    op.run()
    snaps.append(_snapshot(store, op))
    if oracle is not None:
      assert oracle.step(grads) == bool(snaps[-1]["skip"]), step
    if between is not None:
      between(step, store)
  return snaps, store, oracle, cached_tensors


def test_cached_weight_norms_are_the_bits_of_the_pass_that_reads_the_weights(cuda, monkeypatch):
  on, store, oracle, ncached = _trajectory(cuda, monkeypatch, True, ref=True, check=True)
  # the first step reads every tensor's weights; from the second on none (nobody touched the public views)
  assert ncached == [0] + [len(SHAPES)] * 5, ncached
  assert store.wnorm_mismatches() == 0
  assert [s["skip"] for s in on] == [0, 0, 1, 0, 0, 0]
  # the cached run against the NumPy oracle, with the tolerances of tests/test_optimizer_gpu.py::_run
  for p, w in zip(store.params, oracle.w):
    torch.testing.assert_close(p.master.cpu(), torch.from_numpy(w), rtol=2e-4, atol=1e-6)
    torch.testing.assert_close(p.w16.float().cpu(), torch.from_numpy(w).to(torch.bfloat16).float(), rtol=1e-2,
                               atol=1e-3)
  off, _, _, noff = _trajectory(cuda, monkeypatch, False)
  assert noff == [0] * 6, noff              # without the cache every tensor stays "read the weights"
  for step, (a, b) in enumerate(zip(on, off)):
    _equal(a, b, step)


def test_writes_behind_the_optimizer_invalidate_the_cached_norms(cuda, monkeypatch):
  """A write through a variable's public view, a write into the raw buffer followed by refresh_compute_copies(),
  and a write right after a skipped step: the next steps equal the uncached run bit for bit."""
  def between(step, store):
    if step == 0:
      p = store.params[3]
      p.master.copy_(torch.full(p.shape, 0.25, device=p._master.device))
    elif step == 2:                         # (the step with the Inf: skipped)
      store.params[5].master.mul_(1.5)
    elif step == 3:
      store._master.mul_(0.9)               # nobody is told ...
      store.refresh_compute_copies()        # ... until here
  on, store, _, ncached = _trajectory(cuda, monkeypatch, True, between, check=True)
  n = len(SHAPES)
  assert ncached == [0, n - 1, n, n - 1, 0, n], ncached
  assert store.wnorm_mismatches() == 0
  off, _, _, _ = _trajectory(cuda, monkeypatch, False, between)
  for step, (a, b) in enumerate(zip(on, off)):
    _equal(a, b, step)
  assert on[2]["skip"] == 1 and not torch.equal(on[2]["master"], on[3]["master"])


def test_checking_mode_counts_a_stale_cached_norm(cuda, monkeypatch):
  """The control of the checking mode: a write into the raw buffer that nobody is told about IS counted."""
  def between(step, store):
    if step == 1:
      store._master[store.params[4].offset + 7] += 1.0
  _, store, _, _ = _trajectory(cuda, monkeypatch, True, between, nsteps=3, inf_step=-1, check=True)
  assert store.wnorm_mismatches() == 1      # (one chunk holds the element)


SMALL_JASPER_LAYERS = [
    {"type": "conv1d", "repeat": 1, "kernel_size": [11], "stride": [2], "num_channels": 128, "padding": "SAME",
     "dilation": [1], "dropout_keep_prob": 0.9},
    {"type": "conv1d", "repeat": 2, "kernel_size": [11], "stride": [1], "num_channels": 128, "padding": "SAME",
     "dilation": [1], "dropout_keep_prob": 0.9, "residual": True, "residual_dense": True},
    {"type": "conv1d", "repeat": 2, "kernel_size": [13], "stride": [1], "num_channels": 384, "padding": "SAME",
     "dilation": [1], "dropout_keep_prob": 0.9, "residual": True, "residual_dense": True},
    {"type": "conv1d", "repeat": 1, "kernel_size": [1], "stride": [1], "num_channels": 256, "padding": "SAME",
     "dilation": [1], "dropout_keep_prob": 0.9},
]


def _small_models():
  from openseq2seq_amd.configs.jasper import jasper10x5_config
  from openseq2seq_amd.configs.transformer import transformer_config
  cls, p = jasper10x5_config(batch_size_per_gpu=4, use_horovod=False, max_steps=100)
  p["encoder_params"]["convnet_layers"] = copy.deepcopy(SMALL_JASPER_LAYERS)
  yield "jasper", cls, p
  cls, p = transformer_config(d_model=512, num_layers=2, num_heads=8, batch_size_per_gpu=16, vocab_size=1024,
                              max_length=24, max_steps=1000)
  yield "transformer", cls, p


@pytest.mark.parametrize("async_opt", [False, True])
def test_checking_mode_finds_no_stale_norm_in_three_train_steps(cuda, monkeypatch, async_opt):
  """Only the Jasper leg exercises the cache and its check: the small Transformer has no LARC, so no weight norm is
  wanted, nothing is cached and the mismatch counter is never written (asserted below: no optimizer launch asks for
  the mask). That leg shows that the new launch path leaves a model without LARC alone."""
  from openseq2seq_amd.optimizers import flat_params
  monkeypatch.setattr(flat_params, "CACHED_WNORM", True)
  monkeypatch.setattr(flat_params, "CHECK_WNORM", True)
  for name, cls, p in _small_models():
    torch.manual_seed(5); np.random.seed(5); random.seed(5)
    p = copy.deepcopy(p)
    p["os2s_async_optimizer"] = async_opt
    p["random_seed"] = 5
    m = cls(p, mode="train", hvd=None, device=cuda)
    m.compile()
    dl = m.get_data_layer()
    seen, upload = [], m.store.need_w_mask          # the host flags at each optimizer launch

    def need_w_mask(store=m.store, upload=upload):
      seen.append({q.name: q.need_w for q in store.params})
      return upload()
    m.store.need_w_mask = need_w_mask
    for s in range(3):
      m.train_step(dl.synthetic_batch(cuda, seed=60 + s))
    assert m.store.wnorm_mismatches() == 0, name
    assert m.train_op.read_state()["global_step"] == 3, name
    assert len(seen) == (3 if m.train_op.cfg.use_larc else 0), name     # (no LARC: no weight norm, nothing cached)
    if seen:
      # the cache is in use: the convolution kernels (the layers read their bf16 copies only) are not re-read, the
      # BatchNorm vectors the layers read in fp32 every forward pass are
      assert all(seen[0].values()), name
      kinds = {q.name: q.kind for q in m.store.params}
      assert not any(v for k, v in seen[2].items() if kinds[k] == "conv"), name
      assert any(v for k, v in seen[2].items() if kinds[k] == "vector"), name
    del m


def test_masked_fill_zeroes_exactly_the_unmasked_tensors(cuda):
  from openseq2seq_amd import capi
  store, _, _ = _store(cuda)
  store._grads.fill_(float("nan"))
  skip = torch.tensor([i % 2 for i in range(len(SHAPES))], dtype=torch.uint8, device=cuda)
  capi.fill_zero_chunks(store._grads, store.chunk_tensor, skip, store.tensor_chunk_begin, store.tensor_numel)
  torch.cuda.synchronize()
  begins = store.tensor_chunk_begin.cpu().tolist()
  for i, p in enumerate(store.params):
    whole = store._grads[begins[i] * store.chunk:begins[i + 1] * store.chunk]     # with the padding up to the chunk
    assert whole.numel() >= p.numel and whole.numel() % store.chunk == 0 and begins[i] * store.chunk == p.offset
    body, padding = whole[:p.numel], whole[p.numel:]
    if i % 2:
      assert bool(torch.isnan(body).all()), i                    # a skipped tensor keeps the poison in every element
    else:
      assert bool((body.view(torch.int32) == 0).all()), i        # +0.0 in every element
    # the padding up to the chunk boundary is zeroed for both: no producer writes it, the statistics pass reads it
    assert bool((padding.view(torch.int32) == 0).all()), i
