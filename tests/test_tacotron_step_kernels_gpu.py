"""Every dispatch class of the free-running Tacotron 2 decode step (csrc/tacotron_infer.hip: ti_lstm_kernel for
both cells, ti_scores_kernel, ti_context_kernel) against a stage-wise float64 oracle, element by element.
tests/_tacotron_step_cases.py holds the case table, the oracle and compare(); the CPU side of it
(conditions on the inputs, agreement with oracle.tacotron.decoder_infer, mutation checks of compare()) is
tests/test_tacotron_step_oracle_cpu.py.

The host code picks kernels and trip counts by shape; the table holds the smallest shapes that reach each:

  base, keep1                   one 16-sample tile, pre-net dropout on / off
  b16, b17, b29, b32_parts4     NT = 1 / 2 column tiles with padding columns; 8 / 4 context parts; a part of 3 tiles
  s1 ... s544                   S = 1, the 32-position pitch, kTiKs = 8 requested steps exactly (256), the rolled
                                rest (257), a second trip of every 512-strided loop (544; supported() accepts it)
  h512, h576, h1024             either side of the two-piece dot over H, and its limit
  p192_nm128, p256_nm80         RG = 512 / 24 no divisor, n_mel at its limit; nm16 > n_mel (b32_parts4: 24, b17: 8)
  k2048, k2112, k2368, k2624    ti_geom(): 8x4 full, 9x4 with dead slots, 8x5, 8x5 with a second round of one live
                                chunk (and 39 context tiles per part: the rolled tile loop); bf16 and e4m3
  config                        the configuration's sizes (B 32, S 200, H = M = 1024, P 256, 80 mel bins)
  mask_seq_a, mask_seq_b        the stop decision on the device: decoding ends early / a sample never finishes
  zoneout_blend                 the eval-mode zoneout blend of the state stores (tests/test_zoneout_gpu.py compares the
                                fused decode with zoneout by whole-trajectory norms only)

test_forced_geometry runs the shipped experiment switches tacotron_infer.rows = 32 and tacotron_infer.geom
(8x4, 8x5, 9x4, 11x3, 12x3, 16x2, 16x3) on the k2112 shape, bf16 and e4m3, B = 3 and 20, and
tacotron_infer.ctx_parts = 1, 2 on b32_parts4. Two geometries need not agree bit for bit; each meets the oracle.

Per case (compare()): a sentinel in every row the kernels write (rows of run steps hold none, the others keep
it bit for bit), alignments past src_len exactly zero, alignment rows summing to 1 and the cumulative
recurrence within 1e-6, both copies of every h / context row bit-equal, the stop bookkeeping (state[1],
finished, lengths) equal to the reference rule on the device's own stop logits, every stage of every step
within its derived error bound E (fp32: |got - R| <= E; bf16: bf16(R - E) <= got <= bf16(R + E)), a second run
and a steps(0, 1) + steps(1, T) run bit-identical to the first.

Worst err / E observed on the MI355X, per stage (a ratio above 1 fails): RATIOS_OBSERVED below. The bounds
are worst-case chains and the kernels' errors behave like random sums, so the ratios sit well below 1; a bf16
output mostly lands on the rounding of R itself (ratio 0). What the bounds still catch is shown on the CPU:
every mistake of MUTATIONS built into the oracle's own result fails compare().

Found by these tests: no kernel bug. Every case, every forced geometry and both ctx_parts settings met the
bounds; supported() accepted S = 544 and every other shape as the table states it. oracle.tacotron.decoder_infer
rounded bf16 stores through fp32 whatever the input type and so could not run on float64 inputs; it now keeps
the input type."""
import pytest

import _tacotron_step_cases as C

pytestmark = pytest.mark.gpu

# worst err / E per stage over the table and the forced geometries, as the tests printed them on the MI355X when
# this file was written (the tests compute their own at run time)
RATIOS_OBSERVED = {
    "table": dict(prenet=0.010, cell0=0.080, cell1=0.036, q=0.045, mh=0.027, align=0.013, ctx=0.250, mel=0.107,
                  stop=0.000),     # worst: cell0 h1024, q b16, ctx k2112_b20, mel k2368, align config_e4m3
    "forced": dict(cell0=0.059, cell1=0.036, ctx=0.127),   # rows = 32 and every geom on k2112; ctx on b32_parts4
}


def _report(fails):
  assert not fails, "\n".join(fails)


@pytest.mark.parametrize("case", C.TABLE)
def test_step_kernels_vs_stage_oracle(cuda, case):
  ratios = {}
  fails = C.check_case(case, cuda, ratios=ratios)
  print("RATIOS %s %s" % (case, " ".join("%s=%.3f" % (k, ratios[k]) for k in C.STAGES if k in ratios)))
  _report(fails)


@pytest.mark.parametrize("option,value,case,stages", C.FORCED,
                         ids=["%s=%d-%s" % (o.split(".")[1], v, n) for o, v, n, _ in C.FORCED])
def test_forced_geometry(cuda, option, value, case, stages):
  from openseq2seq_amd import _lib
  ratios = {}
  fails = C.check_forced(option, value, case, stages, cuda, ratios=ratios)
  print("RATIOS %s=%d %s %s" % (option, value, case, " ".join("%s=%.3f" % (k, ratios[k]) for k in C.STAGES if k in ratios)))
  for k, v in C.OPTION_DEFAULTS.items():
    assert _lib.get_option(k) == v, (k, _lib.get_option(k))
  _report(fails)
