"""Helpers of the sampled-softmax tests (not a test module).

The sequential candidate sampler (the hash of csrc/os2s_common.hpp, the integer bound table, rejection of repeats,
the try cap and the fill), and the fp64 restatement R of tf.nn.sampled_softmax_loss as include/os2s.h states it
(num_true = 1, log-uniform sampler, unique, accidental hits removed, log Q subtracted), forward and backward, written
with explicit gradients. R_b (`reference(..., rb=True)`) is the same arithmetic with a bf16 round wherever the device
stores bf16: the sampled logits, dlogits, and dX after the GEMM and again after the true-row add (W and x are bf16
values already). TensorFlow is not available here: nothing reference-held pins this restatement."""
import numpy as np
import torch

M64 = (1 << 64) - 1


def hash_u32(seed, idx):
  z = (idx * 0x9E3779B97F4A7C15 + seed) & M64
  z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
  z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
  z = z ^ (z >> 31)
  return z >> 32


def bounds(V):
  """Upper bound (exclusive) of class k in uniform space: floor(2^32 log(k+2) / log(V+1)); the last is 2^32."""
  b = np.floor(np.log(np.arange(2, V + 2, dtype=np.float64)) / np.log(V + 1.0) * 4294967296.0).astype(np.int64)
  b[-1] = 1 << 32
  return b


def draw_classes(V, seed, n, start=0):
  """The classes of tries start .. start + n - 1."""
  b = bounds(V)
  u = np.array([hash_u32(seed, t) for t in range(start, start + n)], dtype=np.int64)
  return np.searchsorted(b, u, side="right")


def sample(V, S, seed, max_tries=None):
  """(ids in draw order, num_tries): the first S distinct classes; at the cap the smallest unsampled ones fill."""
  max_tries = 16 * S + 64 if max_tries is None else max_tries
  b = bounds(V)
  ids, seen, t = [], set(), 0
  while len(ids) < S and t < max_tries:
    k = int(np.searchsorted(b, hash_u32(seed, t), side="right"))
    t += 1
    if k not in seen:
      seen.add(k)
      ids.append(k)
  if len(ids) < S:
    t = max_tries
    k = 0
    while len(ids) < S:
      if k not in seen:
        ids.append(k)
      k += 1
  return np.array(ids, dtype=np.int64), t


def log_q(ids, num_tries, V):
  p = np.log1p(1.0 / (np.asarray(ids, dtype=np.float64) + 1.0)) / np.log(V + 1.0)
  return np.log(-np.expm1(num_tries * np.log1p(-p)))


def bf16(a):
  return torch.from_numpy(np.asarray(a, dtype=np.float64)).float().to(torch.bfloat16).double().numpy()


def reference(x, W, b, labels, ids, num_tries, V, scale, gs=None, rb=False):
  """x [N,D], W [V,D], b [V] fp64; labels [N], ids [S] int. loss = scale * sum(row_loss); gs (default scale)
  multiplies the gradients. Returns a dict of fp64 arrays."""
  gs = scale if gs is None else gs
  rnd = bf16 if rb else (lambda a: a)
  labels, ids = np.asarray(labels, dtype=np.int64), np.asarray(ids, dtype=np.int64)
  true = (x * W[labels]).sum(1) + b[labels] - log_q(labels, num_tries, V)
  samp = rnd(x @ W[ids].T + (b[ids] - log_q(ids, num_tries, V))[None, :])
  hit = ids[None, :] == labels[:, None]
  z = np.concatenate([true[:, None], np.where(hit, -np.inf, samp)], axis=1)
  mx = z.max(1, keepdims=True)
  lse = (mx + np.log(np.exp(z - mx).sum(1, keepdims=True)))[:, 0]
  row_loss = lse - true
  p = np.exp(z - lse[:, None])
  dtrue = gs * (p[:, 0] - 1.0)
  dlogits = rnd(gs * p[:, 1:])
  dx = rnd(rnd(dlogits @ W[ids]) + dtrue[:, None] * W[labels])
  dW = np.zeros_like(W)
  np.add.at(dW, ids, dlogits.T @ x)
  np.add.at(dW, labels, dtrue[:, None] * x)
  db = np.zeros_like(b)
  np.add.at(db, ids, dlogits.sum(0))
  np.add.at(db, labels, dtrue)
  return dict(row_loss=row_loss, loss=scale * row_loss.sum(), dtrue=dtrue, dlogits=dlogits, dx=dx, dW=dW, db=db,
              hit=hit, p=p)


def make_case(N, D, V, S, seed, hits=3):
  """bf16-valued x [N,D], W [V,D], fp32-valued b [V], the sampler's candidate set and labels of which the first
  `hits` rows are sampled ids (accidental hits)."""
  g = np.random.RandomState(seed)
  x = bf16(g.randn(N, D))
  W = bf16(g.randn(V, D) * (1.0 / np.sqrt(D)))
  b = (g.randn(V) * 0.1).astype(np.float32).astype(np.float64)
  ids, tries = sample(V, S, seed)
  labels = g.randint(0, V, size=N)
  labels[:hits] = ids[g.permutation(S)[:hits]]
  labels[hits] = labels[hits + 1] = (labels[0] + 1) % V        # a repeated label: two rows add into one table row
  return dict(x=x, W=W, b=b, ids=ids, tries=tries, labels=labels)


def count_hit_rows(labels, ids):
  return int(np.isin(labels, ids).sum())
