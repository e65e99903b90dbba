"""CPU (gloo, world_size 2): the data-parallel plumbing that replaces Horovod —
bucketed flat-gradient all-reduce (optimizers.py:77-104), rank-0 broadcast of the
variables (hooks.py:15-55), object gather (utils.py:47-82) — and the world-size
averaging convention of the optimizer (gradients are SUMS over ranks; the kernel
divides by world_size)."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


class _Store(object):
  """CPU stand-in for FlatParams (only what the reducer / broadcast touch)."""

  def __init__(self, n, chunk=4096):
    self.chunk = chunk
    self.master = torch.zeros(n)
    self.grads = torch.zeros(n)
    self.refreshed = 0

  def refresh_compute_copies(self):
    self.refreshed += 1


def _free_port():
  s = socket.socket()
  s.bind(("127.0.0.1", 0))
  p = s.getsockname()[1]
  s.close()
  return p


def _worker(rank, world, port, q):
  os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                    WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
  from openseq2seq_amd.utils import distributed as du
  hvd = du.init_from_env(backend="gloo")
  assert hvd.rank() == rank and hvd.size() == world
  n = 4096 * 5 + 0
  st = _Store(n)
  torch.manual_seed(100 + rank)
  st.master.copy_(torch.randn(n))
  extra = torch.full((7,), float(rank))
  du.broadcast_parameters(st, [extra])
  ref = torch.Generator().manual_seed(100)
  torch.manual_seed(100)
  expect_master = torch.randn(n)
  ok_bcast = bool(torch.equal(st.master, expect_master)) and float(extra.sum()) == 0.0 \
      and st.refreshed == 1
  # gradients: rank r holds (r+1) * base -> sum = 3 * base for world 2
  base = torch.arange(n, dtype=torch.float32) / n
  st.grads.copy_(base * (rank + 1))
  red = du.GradientReducer(st, world, bucket_bytes=4096 * 4 * 2)   # forces 3 buckets
  assert len(red.bounds) == 3
  red.all_reduce()
  ok_sum = bool(torch.allclose(st.grads, base * sum(range(1, world + 1))))
  # overlapped form: buckets are reduced as the backward watermark moves down
  st.grads.copy_(base * (rank + 1))
  red.mark_done(4096 * 4 + 7)          # inside the last bucket: nothing complete yet
  ok_sum = ok_sum and red.next_bucket == 2
  red.mark_done(4096 * 4)              # the last bucket [16384, 20480) is complete
  ok_sum = ok_sum and red.next_bucket == 1
  ok_sum = ok_sum and bool(torch.allclose(st.grads[16384:], base[16384:] * 3))
  ok_sum = ok_sum and bool(torch.allclose(st.grads[:16384], base[:16384] * (rank + 1)))
  red.mark_done(4096 * 2)              # bucket [8192, 16384) now complete
  ok_sum = ok_sum and red.next_bucket == 0
  red.finish()
  ok_sum = ok_sum and bool(torch.allclose(st.grads, base * 3)) and red.next_bucket == 2
  # OS2S_ALLREDUCE_DTYPE=bf16: half the bytes on the wire, sums within bf16 rounding (2^-8 relative)
  os.environ["OS2S_ALLREDUCE_DTYPE"] = "bf16"
  red16 = du.GradientReducer(st, world, bucket_bytes=4096 * 4 * 2)
  del os.environ["OS2S_ALLREDUCE_DTYPE"]
  st.grads.copy_(base * (rank + 1))
  red16.all_reduce()
  ok_sum = ok_sum and red16.wire_dtype == torch.bfloat16 and red.wire_dtype == torch.float32
  ok_sum = ok_sum and bool(torch.allclose(st.grads, base * 3, rtol=2 ** -7, atol=1e-6))
  ok_sum = ok_sum and not bool(torch.equal(st.grads, base * 3))      # it really went through bf16
  objs = du.gather_objects({"rank": rank, "n": rank * 10})
  ok_gather = (objs is None) if rank != 0 else ([o["n"] for o in objs] == [0, 10])
  q.put((rank, ok_bcast, ok_sum, ok_gather))
  dist.barrier()
  dist.destroy_process_group()


def test_gloo_world2():
  ctx = mp.get_context("spawn")
  q = ctx.Queue()
  port = _free_port()
  procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
  for p in procs:
    p.start()
  res = [q.get(timeout=120) for _ in range(2)]
  for p in procs:
    p.join(timeout=60)
    assert p.exitcode == 0
  for r in res:
    assert r[1] and r[2] and r[3], r


def test_tape_watermark_waits_for_out_of_order_and_shared_variables():
  """The watermark handed to the reducer only passes a variable once EVERY closure listing it
  has run, whatever the creation order (tied embeddings, a variable created after its consumer)."""
  from openseq2seq_amd.parts.cnns.conv_blocks import Tape

  class P(object):
    def __init__(self, offset):
      self.offset = offset

  emb, l1, l2, late, proj = P(0), P(100), P(200), P(300), P(400)
  marks, ran = [], []
  tape = Tape(on_done=marks.append)
  # forward order: embedding(emb), layer1(l1), [late is created after l2 but used before it],
  # layer `late`, layer2(l2), projection(proj) which also writes the tied emb gradient
  tape.record(lambda: ran.append("emb"), [emb])
  tape.record(lambda: ran.append("l1"), [l1])
  tape.record(lambda: ran.append("late"), [late])
  tape.record(lambda: ran.append("l2"), [l2])
  tape.record(lambda: ran.append("proj"), [proj, emb])
  tape.record(lambda: ran.append("loss"))
  tape.backward()
  assert ran == ["loss", "proj", "l2", "late", "l1", "emb"]
  # after proj: 400 final. after l2: `late` (300) above it is still pending -> no progress.
  # after late: 300 and 200 final -> 200. then 100, then 0 (emb listed twice: final at the end)
  assert marks == [400, 200, 100, 0]
  assert tape.ops == []
  # without a reducer the closures simply run
  t2 = Tape()
  t2.record(lambda: ran.append("x"), [emb])
  t2.backward()
  assert ran[-1] == "x"


# ---- tower mode: `use_horovod False, num_gpus N` (models/model.py:386-427) -------------------

REF_DS2 = "/root/reference/example_configs/speech2text/ds2_large_8gpus.py"
_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _clean_env(**extra):
  env = dict(os.environ)
  for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "GROUP_RANK",
            "LOCAL_WORLD_SIZE", "TORCHELASTIC_RUN_ID"):
    env.pop(k, None)
  env.update(extra)
  return env


def test_plan_workers_rules():
  from openseq2seq_amd.utils.distributed import plan_workers
  # Horovod mode: the launcher decides, num_gpus is ignored (as in the reference)
  assert plan_workers({"use_horovod": True, "num_gpus": 8}, {}) == (1, False)
  assert plan_workers({"use_horovod": True}, {"WORLD_SIZE": "4"}) == (4, False)
  # tower mode: N replicas = N ranks; start them when nobody did
  assert plan_workers({"use_horovod": False, "num_gpus": 8}, {}) == (8, True)
  assert plan_workers({"use_horovod": False, "gpu_ids": [0, 1, 2], "num_gpus": 8}, {}) == (3, True)
  assert plan_workers({"use_horovod": False, "num_gpus": 2}, {"WORLD_SIZE": "2"}) == (2, False)
  assert plan_workers({"use_horovod": False, "num_gpus": 1}, {}) == (1, False)
  assert plan_workers({"use_horovod": False}, {}) == (1, False)
  with pytest.raises(ValueError):      # a launcher that contradicts the config is refused
    plan_workers({"use_horovod": False, "num_gpus": 8}, {"WORLD_SIZE": "2"})
  with pytest.raises(ValueError):
    plan_workers({"use_horovod": False, "num_gpus": 1}, {"WORLD_SIZE": "2"})


@pytest.mark.skipif(not os.path.isfile(REF_DS2), reason="reference checkout not present")
def test_tower_config_starts_its_ranks():
  """The reference's ds2_large_8gpus.py (use_horovod False, num_gpus 8, batch_size_per_gpu 16)
  with num_gpus overridden to 2: run.py starts 2 ranks itself (gloo here), every rank joins, the
  global batch is 32. It never runs the config on one replica."""
  import json
  import subprocess
  import sys
  r = subprocess.run([sys.executable, os.path.join(_REPO, "run.py"), "--config_file=" + REF_DS2,
                      "--mode=train", "--num_gpus=2"],
                     stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600,
                     env=_clean_env(OS2S_LAUNCH_DRY_RUN="1"))
  assert r.returncode == 0, r.stderr[-2000:]
  lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
  assert len(lines) == 1, r.stdout
  d = json.loads(lines[0])
  assert d["world_size"] == 2 and d["ranks_seen"] == 2 and d["global_batch"] == 32
  assert d["use_horovod"] is False and d["backend"] in ("gloo", "nccl")


@pytest.mark.skipif(not os.path.isfile(REF_DS2), reason="reference checkout not present")
def test_tower_config_refuses_a_smaller_world():
  import subprocess
  import sys
  r = subprocess.run([sys.executable, os.path.join(_REPO, "run.py"), "--config_file=" + REF_DS2,
                      "--mode=train"],                        # num_gpus 8 as written
                     stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600,
                     env=_clean_env(OS2S_LAUNCH_DRY_RUN="1", WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"))
  assert r.returncode != 0 and "num_gpus=8" in r.stderr


def test_model_refuses_fewer_replicas_than_the_config_names():
  """Model.__init__ itself (not only run.py) refuses `num_gpus 8` on a one-rank process group;
  Model.num_gpus reports the replica count (model.py:293-303)."""
  from openseq2seq_amd.models.model import Model

  class M(Model):
    def _build_forward_pass_objects(self, store):
      pass

    def _forward_backward(self, batch, tape):
      pass

    def _get_num_objects_per_step(self, batch):
      return 0

  base = {"use_horovod": False, "batch_size_per_gpu": 16, "data_layer": None}
  dev = torch.device("cpu")
  with pytest.raises(ValueError, match="8 replicas"):
    M(dict(base, num_gpus=8), mode="train", device=dev)
  assert M(dict(base, num_gpus=1), mode="train", device=dev).num_gpus == 1

  class Hvd(object):
    def rank(self):
      return 1

    def size(self):
      return 2

  m = M(dict(base, num_gpus=2), mode="train", hvd=Hvd(), device=dev)
  assert m.num_gpus == 2
  assert M(dict(base, use_horovod=True, num_gpus=8), mode="train", hvd=Hvd(), device=dev).num_gpus == 1


def test_tape_deferred_weight_gradients_hold_the_watermark(monkeypatch):
  """A weight gradient handed to Tape.defer_wgrad (grouped launch later) is not final when its
  closure returns: the reducer's watermark waits for the flush, then moves past it."""
  from openseq2seq_amd import capi
  from openseq2seq_amd.parts.tape import Tape, current_tape

  class P(object):
    def __init__(self, offset):
      self.offset = offset

  launched = []
  monkeypatch.setattr(capi, "gemm_wgrad_grouped",
                      lambda items, accumulate=True: launched.append([it["tag"] for it in items]))
  a, b, c, d, e = P(0), P(100), P(200), P(300), P(400)
  marks = []
  tape = Tape(on_done=marks.append)
  x = torch.zeros(1)

  def closure(param, tag, defer):
    def fn():
      assert current_tape() is tape
      if defer:
        current_tape().defer_wgrad(param, dict(x=x, dy=x, dw=x, tag=tag))
    return fn

  for prm, tag, defer in ((a, "a", True), (b, "b", False), (c, "c", True), (d, "d", True), (e, "e", True)):
    tape.record(closure(prm, tag, defer), [prm])
  tape.backward()
  assert current_tape() is None
  # backward order e, d, c (third deferral -> flush e, d, c together), b, a (flushed at the end)
  assert launched == [["e", "d", "c"], ["a"]]
  # after e and d: deferred, nothing final. after c: flush -> 400, 300, 200 final -> 200. b -> 100.
  # a is deferred until the end-of-backward flush -> 0
  assert marks == [200, 100, 0]
