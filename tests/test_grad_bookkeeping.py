"""CPU tests of the host bookkeeping behind the optimizer tail (optimizers/flat_params.py): the per-tensor "read the
weights" flags of the cached weight norms, the gradient epoch and FlatParams.prepare_grad. Plain Python: the store
lives in host memory and the three device calls it makes are replaced by recorders."""
import pytest
import torch


@pytest.fixture
def store(monkeypatch):
  from openseq2seq_amd import capi
  from openseq2seq_amd.optimizers import flat_params
  calls = []
  monkeypatch.setattr(capi, "cast_f32_to_bf16", lambda src, dst: calls.append("cast"))
  monkeypatch.setattr(capi, "conv_weight_dgrad_copy", lambda *a: calls.append("wt"))

  def fill(buf, chunk_tensor, skip, begin, numel):
    calls.append(("fill", bytes(skip.tolist())))
    for c, t in enumerate(chunk_tensor.tolist()):
      if not skip[t]:
        buf[c * 4096:(c + 1) * 4096] = 0
  monkeypatch.setattr(capi, "fill_zero_chunks", fill)
  monkeypatch.setattr(flat_params, "GRAD_OVERWRITE", True)
  s = flat_params.FlatParams(torch.device("cpu"))
  s.add("a/kernel", (3, 16, 8), torch.ones(3, 16, 8), kind="conv").overwrite_first = True
  s.add("a/gamma", (16,), torch.ones(16), kind="vector")
  s.add("b/kernel", (1, 8, 16), torch.ones(1, 8, 16), kind="conv").overwrite_first = True
  s.finalize()
  s.calls = calls
  return s


def test_need_w_flags_follow_the_public_views(store):
  a, g, b = store.params
  assert all(p.need_w for p in store.params)                 # finalize: nothing is cached yet
  assert bytes(store.need_w_mask().tolist()) == b"\x01\x01\x01"
  store.weights_updated()
  assert not any(p.need_w for p in store.params)
  a._master, a._grad, a.w16, a.wt16, a.grad                  # raw views, the bf16 copies, the gradient: no mark
  assert not any(p.need_w for p in store.params)
  g.master                                                   # a read of the public fp32 view: its holder may write
  assert [p.need_w for p in store.params] == [False, True, False]
  assert bytes(store.need_w_mask().tolist()) == b"\x00\x01\x00" and store._need_w_sent == b"\x00\x01\x00"
  sent = store._need_w_dev
  assert store.need_w_mask() is sent                         # an unchanged set is not sent again
  store.weights_updated()
  store.master                                               # the whole buffer
  assert all(p.need_w for p in store.params)
  store.weights_updated()
  store.refresh_compute_copies()
  assert all(p.need_w for p in store.params)


def test_prepare_grad_and_the_gradient_epoch(store):
  a, g, b = store.params
  store._grads.fill_(float("nan"))
  e0 = store.grad_epoch
  store.begin_grad_epoch()
  assert store.grad_epoch == e0 + 1
  assert store.calls[-1] == ("fill", b"\x01\x00\x01")        # the masked fill leaves the two kernels out
  assert bool(torch.isnan(a._grad).all()) and bool((g._grad == 0).all())
  assert store.prepare_grad(g) is True                       # not an overwrite_first gradient: always accumulate
  assert store.prepare_grad(a) is False                      # the first write of the epoch overwrites ...
  assert store.prepare_grad(a) is True                       # ... the second producer adds
  assert bool(torch.isnan(a._grad).all())                    # (prepare_grad itself wrote nothing)
  # a producer that cannot overwrite: zeroed for it, and part of the step-start fill from now on
  assert store.prepare_grad(b, can_overwrite=False) is True
  assert bool((b._grad == 0).all()) and b.overwrite_first is False
  store.begin_grad_epoch()
  assert store.calls[-1] == ("fill", b"\x01\x00\x00")
  # an accumulation window: no new epoch, everybody adds
  assert store.prepare_grad(a) is False and store.prepare_grad(a) is True
  # the asynchronous update zeroed the buffer: a new epoch without a fill
  n = len(store.calls)
  store.begin_grad_epoch(already_zeroed=True)
  assert len(store.calls) == n and store.prepare_grad(a) is False


def test_unwritten_and_foreign_gradients(store, monkeypatch):
  from openseq2seq_amd.optimizers import flat_params
  a, g, b = store.params
  store._grads.fill_(float("nan"))
  store.begin_grad_epoch()
  assert store.prepare_grad(a) is False
  a._grad.fill_(3.0)                                         # (the producer's write)
  store.finish_grad_epoch()                                  # b: a layer the step did not run
  assert bool((a._grad == 3.0).all()) and bool((b._grad == 0).all()) and b.overwrite_first
  assert store.prepare_grad(b) is True                       # a late producer adds to the zeros
  # the public view of a gradient nobody wrote yet: zeros, and the layer's producer then adds
  store._grads.fill_(float("nan"))
  store.begin_grad_epoch()
  assert bool((a.grad == 0).all()) and a.overwrite_first and store.prepare_grad(a) is True
  # the full fill starts an epoch too
  e = store.grad_epoch
  store.zero_grads()
  assert store.grad_epoch == e + 1 and store.prepare_grad(a) is False
  # option off: the step start fills everything, everybody accumulates
  monkeypatch.setattr(flat_params, "GRAD_OVERWRITE", False)
  store._grads.fill_(float("nan"))
  n = len(store.calls)
  store.begin_grad_epoch()
  assert len(store.calls) == n and bool((store._grads == 0).all())
  assert store.prepare_grad(a) is True and store.prepare_grad(b) is True
  store.finish_grad_epoch()


def test_unwritten_gradients_are_zeroed_as_backward_declares_ranges_final(store):
  """The order a gradient reducer needs: finish_grad_epoch(offset) zeroes the unwritten overwrite_first gradients at
  flat offsets >= offset — before that range is all-reduced —, each variable once, and leaves the rest for later."""
  a, g, b = store.params
  assert a.offset < g.offset < b.offset
  store._grads.fill_(float("nan"))
  store.begin_grad_epoch()
  store.finish_grad_epoch(b.offset)                          # backward has passed b's layer: nobody wrote it
  assert bool((b._grad == 0).all()) and bool(torch.isnan(a._grad).all())
  assert store.prepare_grad(a) is False                      # a's layer runs later in backward and overwrites
  a._grad.fill_(2.0)
  store.finish_grad_epoch(a.offset)
  store.finish_grad_epoch(0)
  assert bool((a._grad == 2.0).all()) and bool((b._grad == 0).all())


def test_switches_are_read_when_used(store, monkeypatch):
  from openseq2seq_amd.optimizers import flat_params
  a = store.params[0]
  for name, fn, var, off, on in (("GRAD_OVERWRITE", flat_params.grad_overwrite, "OS2S_GRAD_OVERWRITE", "0", "1"),
                                 ("CACHED_WNORM", flat_params.cached_wnorm, "OS2S_OPT_CACHED_WNORM", "0", "1"),
                                 ("CHECK_WNORM", flat_params.check_wnorm, "OS2S_OPT_CHECK_WNORM", "0", "1")):
    monkeypatch.setattr(flat_params, name, None)             # nothing set in the process: the environment, each time
    monkeypatch.setenv(var, off)
    assert fn() is False
    monkeypatch.setenv(var, on)
    assert fn() is True
    monkeypatch.setattr(flat_params, name, False)            # an explicit setting wins
    assert fn() is False
  monkeypatch.setattr(flat_params, "GRAD_OVERWRITE", None)
  monkeypatch.setenv("OS2S_GRAD_OVERWRITE", "0")
  store.begin_grad_epoch()
  assert store.prepare_grad(a) is True and store.calls[-1] != ("fill", b"\x01\x00\x01")
  monkeypatch.setenv("OS2S_GRAD_OVERWRITE", "1")
  store.begin_grad_epoch()
  assert store.calls[-1] == ("fill", b"\x01\x00\x01") and store.prepare_grad(a) is False


def test_single_owner_query_is_the_launchers_decision():
  """os2s_conv1d_wgrad_single_owner: the envelope of the kernels with one owner per dW element, options included
  (host code only: no device call)."""
  from openseq2seq_amd import _lib
  q = _lib.C.os2s_conv1d_wgrad_single_owner

  def ask(B, T, Cin, Cout, K, stride=1, dil=1):
    tout = -(-T // stride)
    return q(B, T, Cin, Cout, K, stride, dil, tout, Cin)
  assert ask(32, 840, 768, 768, 25) == 1 and ask(32, 840, 896, 1024, 29, dil=2) == 1     # Jasper's wide layers
  assert ask(32, 1680, 64, 256, 11, stride=2) == 0            # the strided first layer: lockstep
  assert ask(32, 840, 1024, 1024, 1) == 0                     # K = 1
  assert ask(32, 840, 256, 64, 11) == 0 and ask(32, 840, 32, 256, 11) == 0      # narrow
  assert ask(65, 840, 768, 768, 25) == 0                      # more samples than the step table holds
  assert ask(3, 24, 128, 128, 5) == 0                         # two units: under conv1d_wgrad.pp_min_units
  old = _lib.get_option("conv1d_wgrad.pp_min_units"), _lib.get_option("conv1d_wgrad.variant")
  try:
    _lib.set_option("conv1d_wgrad.pp_min_units", 1)
    assert ask(3, 24, 128, 128, 5) == 1
    _lib.set_option("conv1d_wgrad.variant", 0)                # the ping-pong kernel switched off
    assert ask(3, 24, 128, 128, 5) == 0 and ask(32, 840, 768, 768, 25) == 0
  finally:
    _lib.set_option("conv1d_wgrad.pp_min_units", old[0])
    _lib.set_option("conv1d_wgrad.variant", old[1])
