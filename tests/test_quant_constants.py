"""The constants ``test_gpu_ecquant.py`` places its row and column lengths on, read from the kernel source: a retune that moves one fails
here, naming the boundary test to rebuild around the new value (in the manner of ``test_select_constants.py``)."""
import os
import re

import pytest

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "alntools_amd", "csrc", "quant.inc")

PINNED = [
    ("Q_LONG_ROW", "256", "test_rows_and_columns_around_the_thresholds (a row with more non-zeros is summed by a workgroup)"),
    ("Q_LONG_COL", "32", "test_rows_and_columns_around_the_thresholds (a column with more entries is summed by a workgroup of its own, all its haplotypes at once)"),
    ("Q_BATCH", "8", "test_the_run_stops_at_the_checkers_step (steps enqueued between two looks at the device)"),
]
Q_LONG_ROW, Q_LONG_COL, Q_BATCH = 256, 32, 8             # what the GPU tests import


def _source():
    with open(SRC) as f:
        return f.read()


@pytest.mark.parametrize("name,value,test", PINNED, ids=[p[0] for p in PINNED])
def test_constants_the_ecquant_tests_straddle(name, value, test):
    defs = re.findall(r"constexpr\s+u32\s+%s\s*=\s*([^;,]+);" % name, _source())
    assert len(defs) == 1, "%d definitions of %s" % (len(defs), name)
    assert defs[0].strip() == value, ("%s is now %s (was %s): move the inputs of test_gpu_ecquant.py::%s onto the new value"
                                      % (name, defs[0].strip(), value, test))


def test_the_thresholds_are_the_ones_the_kernels_branch_on_and_the_sums_are_folded_by_the_workgroup():
    src = _source()
    assert len(re.findall(r"b - a <= Q_LONG_ROW", src)) == 1 and len(re.findall(r"b - a > Q_LONG_ROW", src)) == 1
    assert len(re.findall(r"> Q_LONG_COL", src)) == 2
    assert "atomicAdd(reinterpret_cast<double" not in src and "unsafeAtomicAdd" not in src        # no float atomics
    assert (Q_LONG_ROW, Q_LONG_COL, Q_BATCH) == (256, 32, 8)
