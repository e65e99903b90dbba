# AWD-style LSTM language model at the sizes of the reference's lm/lstm-wkt2-fp32.py (3 LayerNorm-LSTM layers of
# 896 units, embedding 256 tied to the output layer, batch 160, bptt 96, Adam 4e-4, the config's dropout values) on
# a synthetic corpus of about 33 k words generated on the fly; no dataset files needed.
#   python run.py --config_file=example_configs/lm/lstm_lm_synthetic.py --mode=train --benchmark --bench_steps=30
import os
import tempfile

from open_seq2seq.configs.lstm_lm import lstm_lm_config
from open_seq2seq.data.lm.synthetic import write_zipf_corpus

_root = os.path.join(tempfile.gettempdir(), "os2s_lm_synthetic_%d" % os.getuid())
if not os.path.exists(os.path.join(_root, "raw", "test.txt")):
  write_zipf_corpus(os.path.join(_root, "raw"))

base_model, base_params, train_params, eval_params, infer_params = lstm_lm_config(
    os.path.join(_root, "raw"), os.path.join(_root, "processed"), seed_tokens="w0 w1 w2")
base_params["print_loss_steps"] = 10
