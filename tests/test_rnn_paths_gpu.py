"""Every dispatch class of the recurrence kernels (csrc/rnn.hip, csrc/rnn_xcd.hip, csrc/rnn_tile.hpp) against
the float64 oracle of tests/_rnn_cases.py, whose docstring lists the kernel instance each case reaches and
states the bound: |got - R_b| <= 4 n_q + 2^-7 |R_b| elementwise on y, the saved gates, c_seq, dgx and dgr,
exact zeros past the lengths, untouched guard columns in the strided runs. tests/test_rnn_oracle_cpu.py
shows on the CPU that the bound rejects seven wrong recurrences.

GRU cases of the step kernels run under os2s_gru_xcd_set_mode(0); persistent cases run at the default mode,
must raise os2s_gru_xcd_launch_count() by the number of persistent launches the table expects (forward, and
backward where it is persistent), leave os2s_gru_xcd_status() at 0 and repeat bit-identically on live rows.
On a device the persistent kernels do not select (not 256 compute units) those cases skip, with the reason.

The helper's docstring carries n_q and the largest err / bound per case and output as measured on the MI355X
when this file was written (largest of all: 0.27, rows32_h72-lstm_cudnn gates); the tests compute their own
n_q. Every persistent case raised the launch count by the expected number and left the status word at 0;
x_b17_h840 (163 466 B of dynamic LDS) launched."""
import pytest

import _rnn_cases as C


@pytest.mark.gpu
@pytest.mark.parametrize("case,cell", C.RUNS, ids=["%s-%s" % r for r in C.RUNS])
def test_rnn_paths(cuda, case, cell):
  fails, skip = C.check_case(case, cell, cuda)
  assert not fails, "\n".join(fails)
  if skip:
    pytest.skip(skip)
