"""MXFP8 residual block end in one launch (csrc/conv1d_block_end_mx.hip): the kernel against the fp64 sum of the
dequantised operands within the worst-case fp32 summation bound, R = 0 against os2s_conv1d_fwd_mx bit for bit, the
refusals of the C ABI, and the 'mxfp8_inference' switch at a block end of conv_bn_res_bn_actv / TDNNEncoder."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _mx_ref(x):
  """The format rule on the CPU (as tests/test_conv1d_mx_gpu.py): bf16 [rows, K] -> (e4m3 bytes, scale bytes in the
  device layout [ceil(K/128), rows, 4], the dequantised values in fp64)."""
  rows, K = x.shape
  xb = x.double().view(rows, K // 32, 32)
  amax = xb.abs().amax(-1)
  _, ex = torch.frexp(amax)
  byte = torch.where(amax > 0, (ex - 1 - 8 + 127).clamp(0, 254), torch.zeros_like(ex)).to(torch.int32)
  q = torch.ldexp(xb, (127 - byte)[..., None]).clamp(-448.0, 448.0).float().to(torch.float8_e4m3fn)
  deq = torch.ldexp(q.double(), (byte - 127)[..., None]).view(rows, K)
  KT = (K + 127) // 128
  sc = torch.zeros((rows, KT * 4), dtype=torch.uint8)
  sc[:, :K // 32] = byte.to(torch.uint8)
  return q.view(torch.uint8).view(rows, K), sc.view(rows, KT, 4).permute(1, 0, 2).contiguous(), deq


def _operand(n_outer, n_inner, C, g, shift):
  """bf16 [n_outer * n_inner, C] with a power-of-two magnitude of its own per (outer, inner, 32-block): a scale routed
  from the wrong row, block, tap or source moves an output by 2x or more."""
  r = torch.arange(n_outer * n_inner)[:, None]
  blk = torch.arange(C // 32)[None, :]
  mag = torch.exp2(((r % n_inner + 3 * blk + 5 * (r // n_inner) + shift) % 13 - 6).float()).repeat_interleave(32, dim=1)
  mant = 1.0 + torch.rand((n_outer * n_inner, C), generator=g)
  sign = torch.where(torch.rand((n_outer * n_inner, C), generator=g) < 0.5, -1.0, 1.0)
  return (mag * mant * sign).to(torch.bfloat16)


def _end_ref(x, w, srcs, dil, pad_left, lens, shift, act, f32=False):
  """(fp64 reference, elementwise bound) of a block end. x [B,T,Cin], w [K,Cout,Cin], srcs [(s [B,T,C], v [Cout,C])],
  all fp64. Bound: N 2^-22 (|a| . |w|) with N = Cin K + sum C_r — worst-case fp32 summation with one bit for a
  truncating accumulator — plus 2^-8 |ref| for a bf16 result."""
  B, T, Cin = x.shape
  K = w.shape[0]
  x = x.clone()
  for b, n in enumerate(lens if lens is not None else []):
    x[b, n:] = 0.0
  xp = torch.nn.functional.pad(x, (0, 0, pad_left, (K - 1) * dil - pad_left))
  ref = sum(xp[:, k * dil:k * dil + T] @ w[k].t() for k in range(K)) + sum(s @ v.t() for s, v in srcs)
  mag = sum(xp[:, k * dil:k * dil + T].abs() @ w[k].abs().t() for k in range(K)) + \
      sum(s.abs() @ v.abs().t() for s, v in srcs)
  ref = ref + shift.double()
  if act == 1:
    ref = ref.clamp_min(0.0)
  for b, n in enumerate(lens if lens is not None else []):
    ref[b, n:] = 0.0
  bound = (Cin * K + sum(s.shape[2] for s, _ in srcs)) * 2.0 ** -22 * mag
  return ref, bound if f32 else bound + 2.0 ** -8 * ref.abs()


def _check(out, ref, bound):
  err = (out.double().cpu() - ref).abs()
  print("max err / bound = %.3g" % float((err / bound.clamp_min(1e-300)).max()))
  assert bool((err <= bound).all())


def _case(cuda, B, T, lens, Cin, Cout, K, dil, widths, act, f32):
  """Operands of one kernel case on the device and dequantised: (kwargs of the wrapper, arguments of _end_ref)."""
  from openseq2seq_amd import capi
  g = torch.Generator().manual_seed(B + 3 * T + 5 * Cin + 7 * K + len(widths))
  xq, xs, x_deq = _mx_ref(_operand(B, T, Cin, g, 0))
  wq, ws, w_deq = _mx_ref(_operand(K, Cout, Cin, g, 5))
  dev, deq = [], []
  for r, C in enumerate(widths):
    sq, ss, s_deq = _mx_ref(_operand(B, T, C, g, 2 + r))
    vq, vs, v_deq = _mx_ref(_operand(1, Cout, C, g, 7 + 3 * r))
    dev.append((sq.view(B, T, C).to(cuda), ss.to(cuda), vq.to(cuda), vs.to(cuda)))
    deq.append((s_deq.view(B, T, C), v_deq))
  shift = torch.randn(Cout, generator=g) * 8.0
  ln = torch.tensor(lens, dtype=torch.int32, device=cuda) if lens else None
  _, pad_left = capi.same_padding(T, K, 1, dil)
  args = (xq.view(B, T, Cin).to(cuda), xs.to(cuda), wq.to(cuda), ws.to(cuda))
  kw = dict(k=K, dil=dil, in_len=ln, out_len=ln, ch_shift=shift.to(cuda), act=act, out_f32=f32)
  return args, dev, kw, (x_deq.view(B, T, Cin), w_deq.view(K, Cout, Cin), deq, dil, pad_left, lens, shift, act, f32)


@pytest.mark.parametrize("B,T,lens,Cin,Cout,K,dil,widths,act,f32", [
    (2, 40, None, 64, 8, 3, 1, (64,), 0, False),                          # smallest: half tiles everywhere
    (2, 300, [300, 130], 192, 264, 5, 2, (64, 128, 320), 1, False),       # 2 row tiles, one partly live; 2nd column
                                                                          # tile partial; 128 + 64 tails everywhere
    (3, 258, [258, 3, 0], 128, 40, 1, 1, (64,) * 16, 0, True),            # 16 sources; a dead tile; an empty sample
    (2, 50, [50, 21], 64, 72, 4, 1, (256,), 1, False)])                   # even K (SAME pads right), a wide source
def test_block_end_against_fp64(cuda, B, T, lens, Cin, Cout, K, dil, widths, act, f32):
  from openseq2seq_amd import capi
  args, srcs, kw, ref_args = _case(cuda, B, T, lens, Cin, Cout, K, dil, widths, act, f32)
  out = capi.conv1d_block_end_fwd_mx(*args, srcs, **kw)
  assert out.dtype == (torch.float32 if f32 else torch.bfloat16) and tuple(out.shape) == (B, T, Cout)
  _check(out, *_end_ref(*ref_args))
  for b, n in enumerate(lens or []):
    assert not bool(out[b, n:].any())                   # rows at or past out_len: exactly zero


def test_no_sources_is_conv1d_fwd_mx(cuda):
  """R = 0: the main steps keep os2s_conv1d_fwd_mx's order, so its bits."""
  from openseq2seq_amd import capi
  args, _, kw, _ = _case(cuda, 2, 300, [300, 130], 192, 264, 5, 2, (), 1, False)
  assert torch.equal(capi.conv1d_block_end_fwd_mx(*args, [], **kw), capi.conv1d_fwd_mx(*args, ch_scale=None, **kw))


def test_refusals(cuda):
  from openseq2seq_amd import _lib, capi
  f = _lib.lib().os2s_conv1d_block_end_fwd_mx           # the library's own attribute: returns the status
  p = torch.zeros(1 << 16, dtype=torch.uint8, device=cuda).data_ptr()

  def call(R=1, C=64, sq=p):
    arr = (capi._MxResSrc * 17)()
    for s in arr:
      s.sq, s.s_scale, s.vq, s.v_scale, s.C = sq, p, p, p, C
    return f(None, p, p, p, p, arr, R, p, None, None, None, 1, 16, 64, 8, 3, 1, 1, 16, 16 * 8, 8, 0, 0, -1)
  assert call() == 0 and call(R=16) == 0
  for bad in (dict(R=17), dict(C=32), dict(C=96)):
    assert call(**bad) == -3                            # OS2S_ERR_UNSUPPORTED
  assert call(sq=None) == -1                            # OS2S_ERR_INVALID_ARG
  torch.cuda.synchronize()


def _randomise(layers, g):
  for L in layers:
    L.gamma.master.copy_(0.5 + torch.rand(L.cout, generator=g))
    L.beta.master.copy_(torch.randn(L.cout, generator=g) * 0.2)
    L.moving_mean.copy_(torch.randn(L.cout, generator=g) * 0.1)
    L.moving_var.copy_(0.5 + torch.rand(L.cout, generator=g))


def _model(main, res, x, srcs, lens_h, act=1):
  """fold -> quantise -> accumulate -> shift -> activation -> mask of one block end in fp64. x, srcs: bf16 on the CPU."""
  def fold(L):
    scale = L.gamma.master.cpu().float() / torch.sqrt(L.moving_var.cpu() + L.eps)
    w = (L.kernel.w16.cpu().float() * scale[None, :, None]).to(torch.bfloat16)
    return (_mx_ref(w.view(L.k * L.cout, L.cin))[2].view(L.k, L.cout, L.cin),
            L.beta.master.cpu().float() - L.moving_mean.cpu() * scale)
  deq = lambda t: _mx_ref(t.reshape(-1, t.shape[2]))[2].view(t.shape)
  w, shift = fold(main)
  folded = [fold(br) for br in res]
  shift = torch.stack([shift] + [f[1] for f in folded]).sum(0)
  _, pad_left = main.out_geometry(x.shape[1])
  return _end_ref(deq(x), w, [(deq(s), f[0][0]) for s, f in zip(srcs, folded)], main.dil, pad_left, lens_h, shift, act)


def test_layer_switch(cuda):
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  from openseq2seq_amd.parts.cnns.conv_blocks import ConvBN, conv_bn_res_bn_actv
  from openseq2seq_amd.parts.tape import Act, Tape
  g = torch.Generator().manual_seed(3)
  torch.manual_seed(3)
  store = FlatParams(cuda)
  main = ConvBN(store, "c", "c/bn", 64, 128, 11)
  res = [ConvBN(store, "r0", "r0/bn", 64, 128, 1), ConvBN(store, "r1", "r1/bn", 192, 128, 1)]
  store.finalize()
  _randomise([main] + res, g)
  lens_h = [50, 21, 7]
  lens = torch.tensor(lens_h, dtype=torch.int32, device=cuda)
  hs = [torch.randn((3, 50, c), generator=g).to(torch.bfloat16) for c in (64, 64, 192)]
  for h in hs:
    for b, n in enumerate(lens_h):
      h[b, n:] = 0

  def run(training=False, tape=None, drop=False):
    x, r0, r1 = [Act(h.to(cuda), lens, requires_grad=False) for h in hs]
    return conv_bn_res_bn_actv(main, res, x, [r0, r1], lens, "relu", training, tape, drop_block_prob=0.5 if drop else 0.0,
                               drop_block=drop).data
  bf16, bf16_tape, bf16_drop = run(), run(tape=Tape()), run(drop=True)
  main.mxfp8 = True
  y = run()
  _check(y, *_model(main, res, hs[0], hs[1:], lens_h))
  assert not torch.equal(y, bf16)                       # it is the other path
  assert torch.equal(run(tape=Tape()), bf16_tape) and torch.equal(run(drop=True), bf16_drop)
  main.mxfp8 = False
  assert torch.equal(run(), bf16)                       # the switch off: nothing of the cached copies leaks
  main.mxfp8 = True
  # the folded copies follow the weights (the store's version counter) and the moving statistics
  res[1].kernel.master.mul_(2.0)
  store.refresh_compute_copies()
  _check(run(), *_model(main, res, hs[0], hs[1:], lens_h))
  res[0].moving_var.mul_(4.0)
  main.moving_mean.add_(1.0)
  _check(run(), *_model(main, res, hs[0], hs[1:], lens_h))
  main.mxfp8 = False
  train_bf16 = run(training=True)                       # (training last: its kernels move the moving statistics)
  main.mxfp8 = True
  assert torch.equal(run(training=True), train_bf16)
  _check(run(), *_model(main, res, hs[0], hs[1:], lens_h))       # ... and the folded copies follow that too


@pytest.mark.parametrize("c2", [192, 640])
def test_dense_residual_encoder_switch(cuda, c2):
  """Two dense-residual blocks of one layer each: block end 1 reads (features), block end 2 reads (features, y1).
  The one-block encoder has the same first block (same seed, same creation order) and gives y1. c2 = 192: both ends
  fused. c2 = 640: a width mx_block_end_wins keeps on the dense-residual pass, which then gets both sources but
  evaluates the second end only."""
  from openseq2seq_amd.optimizers.flat_params import FlatParams
  from openseq2seq_amd.encoders.tdnn_encoder import TDNNEncoder
  from openseq2seq_amd.parts.cnns.conv_blocks import conv_bn_dres_actv
  from openseq2seq_amd.parts.tape import Act, Tape
  blk = lambda k, c: dict(type="conv1d", repeat=1, kernel_size=[k], stride=[1], num_channels=c, padding="SAME",
                          dilation=[1], residual=True, residual_dense=True)
  layers = [blk(5, 128), blk(3, c2)]
  lens_h = [300, 257, 9]
  x = torch.randn((3, 300, 64), generator=torch.Generator().manual_seed(5)).to(torch.bfloat16)
  for b, n in enumerate(lens_h):
    x[b, n:] = 0

  def run(n=2, mode="eval", tape=None, **extra):
    torch.manual_seed(0)
    store = FlatParams(cuda)
    enc = TDNNEncoder(dict({"convnet_layers": layers[:n], "dropout_keep_prob": 1.0, "activation_fn": "relu",
                            "use_conv_mask": True, "dtype": "mixed"}, **extra), None, mode=mode).build(store, 64)
    store.finalize()
    _randomise([br for L in enc._layers for br in [L["main"]] + L["res"]], torch.Generator().manual_seed(7))
    src = [x.to(cuda), torch.tensor(lens_h, dtype=torch.int32, device=cuda)]
    return enc, enc.encode({"source_tensors": src, "tape": tape})["outputs"]
  _, off = run()
  _, y1 = run(1, mxfp8_inference=True)
  enc, on = run(mxfp8_inference=True)
  end = enc._layers[1]
  # (the encoder's last layer is not masked: rows past the lengths are act(shift), so the model gets no mask either)
  _check(y1, *_model(enc._layers[0]["main"], enc._layers[0]["res"], x, [x], None))
  y1m = y1.cpu().clone()
  for b, n in enumerate(lens_h):
    y1m[b, n:] = 0
  if c2 == 192:
    _check(on, *_model(end["main"], end["res"], y1m, [x, y1m], None))
  else:             # the parent's own block end on the same two sources, bit for bit
    lens = torch.tensor(lens_h, dtype=torch.int32, device=cuda)
    acts = [Act(t.to(cuda), lens, requires_grad=False) for t in (x, y1m)]
    dpass = enc._dres_plan.begin(False)
    for a in acts:
      dpass.add_source(a)
    assert torch.equal(on, conv_bn_dres_actv(end["main"], acts[1], dpass.forward_end(1), None, "relu", False, None).data)
  assert not torch.equal(on, off)
  assert torch.equal(run(tape=Tape(), mxfp8_inference=True)[1], run(tape=Tape())[1])
  assert torch.equal(run(mode="train", mxfp8_inference=True)[1], run(mode="train")[1])
