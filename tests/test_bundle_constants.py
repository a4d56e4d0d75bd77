"""The constants ``test_gpu_ecbundle.py`` places its runs and pair counts on, read from the kernel source: a retune that moves one fails
here, naming the boundary test to rebuild around the new value (in the manner of ``test_count_constants.py``)."""
import os
import re

import pytest

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "alntools_amd", "csrc", "ecb.hip")

PINNED = [
    ("BD_FOLD_TPB", "TPB", "test_runs_on_the_wave_and_workgroup_boundaries_of_the_fold (workgroups of 256 sorted pairs)"),
    ("BD_WAVE", "64", "test_runs_on_the_wave_and_workgroup_boundaries_of_the_fold (waves of 64 sorted pairs)"),
    ("TPB", "256", "test_runs_on_the_wave_and_workgroup_boundaries_of_the_fold"),
    ("SCB_TPB", "1024", "test_pair_counts_on_the_scan_tile (SCB = SCB_TPB * SCB_ITEMS = 16 384)"),
    ("SCB_ITEMS", "16", "test_pair_counts_on_the_scan_tile (SCB = SCB_TPB * SCB_ITEMS = 16 384)"),
    ("INL", "5", "test_rows_around_the_inline_pair_limit"),
    ("BD_MAX_GROUPS_PER_LOCUS", "65535", "test_refusals (a locus in 65 536 groups)"),
]
FOLD_TPB, WAVE, SCAN_TILE, INL = 256, 64, 16384, 5       # what the GPU tests import


def _source():
    with open(SRC) as f:
        return f.read()


@pytest.mark.parametrize("name,value,test", PINNED, ids=[p[0] for p in PINNED])
def test_constants_the_ecbundle_tests_straddle(name, value, test):
    defs = re.findall(r"constexpr\s+(?:u32|int)\s+(?:\w+\s*=\s*[^;,]+,\s*)*%s\s*=\s*([^;,]+)[;,]" % name, _source())
    assert len(defs) == 1, "%d definitions of %s" % (len(defs), name)
    assert defs[0].strip() == value, ("%s is now %s (was %s): move the inputs of test_gpu_ecbundle.py::%s onto the new value"
                                      % (name, defs[0].strip(), value, test))


def test_the_fold_kernel_is_launched_with_its_own_workgroup_and_the_scan_tile_is_the_product():
    src = _source()
    assert len(re.findall(r"k_bd_fold<<<nblk\(X, BD_FOLD_TPB\), BD_FOLD_TPB, 0, st>>>", src)) == 1
    assert len(re.findall(r"SCB = SCB_TPB \* SCB_ITEMS;", src)) == 1
    assert (FOLD_TPB, WAVE, SCAN_TILE) == (256, 64, 1024 * 16)
