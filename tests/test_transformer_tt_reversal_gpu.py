"""The reference's Transformer acceptance configuration, unchanged (example_configs/text2text/toy-reversal/
nmt-reversal-TT.py: d_model 128, 8 heads of 16, 14-token vocabularies without padding), through run.py's train loop
exactly as test_transformer_learns_reversal_with_beam_search (tests/test_nmt_reversal_gpu.py) runs the 512-wide
variant: 10 000 / 256 / 8 lines, deterministic kernels, fixed seeds, the config's own 800 steps; eval BLEU > 0.9 on
the 256 dev lines (the project's bar for every toy-reversal test and the reference's acceptance criterion), then
infer mode (beam 5) from the checkpoint: at least 6 of the 8 test lines reversed exactly.

Measured on an MI355X (bf16 compute, deterministic kernels). At the config's own 800 steps both seeds clear the BLEU
bar — seed 7: BLEU 0.984 (exact match 0.76), seed 11: BLEU 0.975 (exact match 0.65) — but seed 11 reverses only 5 of
the 8 test lines exactly, one short of the infer bar. Neither the bar nor the config changes: the test passes
--max_steps=2000 on its command line, the most the task allows.
At 2000 steps — seed 7: BLEU 0.991 (exact match 0.83), seed 11: BLEU 0.994 (exact match 0.86) — both seeds clear
both bars; a seed takes 17 s."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_STEPS = 2000     # --max_steps on the command line; the config's own is 800 (see the module docstring)


@pytest.fixture(autouse=True)
def _deterministic_kernels():
  from openseq2seq_amd import capi
  prev = capi.deterministic()
  capi.set_deterministic(True)
  try:
    yield
  finally:
    capi.set_deterministic(prev)


@pytest.mark.parametrize("seed", [7, 11])
def test_tt_config_learns_reversal(cuda, tmp_path, monkeypatch, seed):
  sys.path.insert(0, REPO)
  import run
  from openseq2seq_amd.test_utils.create_reversed_examples import create_data
  from openseq2seq_amd.utils.utils import create_model, get_base_config
  monkeypatch.chdir(tmp_path)
  create_data(train_corpus_size=10000, dev_corpus_size=256, test_corpus_size=8,
              data_path="toy_text_data", seed=0)
  cfg = os.path.join(REPO, "example_configs/text2text/toy-reversal/nmt-reversal-TT.py")
  args, base_config, base_model, config_module = get_base_config(
      ["--config_file=" + cfg, "--mode=train_eval", "--max_steps=%d" % MAX_STEPS, "--print_loss_steps=200",
       "--eval_steps=10000", "--print_samples_steps=10000", "--save_summaries_steps=10000"])
  base_config["random_seed"] = seed
  model = create_model(args, base_config, config_module, base_model, None)
  run.train(model, args)
  res = run.run_eval(model, model.eval_model, 0)
  print("TT reversal, seed %d, %d steps: %r" % (seed, MAX_STEPS, res))
  assert res["samples"] == 256
  assert res["bleu"] > 0.9, res
  args, base_config, base_model, config_module = get_base_config(
      ["--config_file=" + cfg, "--mode=infer", "--infer_output_file=out.txt"])
  imodel = create_model(args, base_config, config_module, base_model, None)
  run.restore_latest(imodel, 0)
  run.infer(imodel, args, 0)
  src = [l.split() for l in open("toy_text_data/test/source.txt").read().strip().splitlines()]
  hyp = [l.split() for l in open("out.txt").read().strip().splitlines()]
  assert len(hyp) == len(src) == 8
  assert sum(h == list(reversed(s_)) for h, s_ in zip(hyp, src)) >= 6, (hyp, src)
