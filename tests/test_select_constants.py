"""The constants ``test_gpu_ecselect.py`` places its sizes on, read from the kernel source: a retune that moves one fails here, naming the
boundary test to rebuild around the new value (in the manner of ``test_bundle_constants.py``)."""
import os
import re

import pytest

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "alntools_amd", "csrc", "ecb.hip")

PINNED = [
    ("SEL_TPB", "256", "test_rows_across_the_work_boundaries and test_columns_across_the_work_boundaries (a workgroup's share: SEL_TPB * SEL_ITEMS entries)"),
    ("SEL_ITEMS", "4", "test_rows_across_the_work_boundaries and test_columns_across_the_work_boundaries (a thread's share)"),
]
SCAN = [("SCB_TPB", "1024"), ("SCB_ITEMS", "16"), ("TPB", "256")]       # test_sizes_on_the_scans_stretch: SCB = SCB_TPB * SCB_ITEMS = 16 384
SCAN_TILE, SEL_TPB, SEL_ITEMS = 16384, 256, 4            # what the GPU tests import
SHARE = SEL_TPB * SEL_ITEMS                              # entries of A or N per workgroup of the passes and gathers


def _source():
    with open(SRC) as f:
        return f.read()


def _pinned(name, value, test):
    defs = re.findall(r"constexpr\s+(?:u32|int)\s+(?:\w+\s*=\s*[^;,]+,\s*)*%s\s*=\s*([^;,]+)[;,]" % name, _source())
    assert len(defs) == 1, "%d definitions of %s" % (len(defs), name)
    assert defs[0].strip() == value, ("%s is now %s (was %s): move the inputs of test_gpu_ecselect.py::%s onto the new value"
                                      % (name, defs[0].strip(), value, test))


@pytest.mark.parametrize("name,value,test", PINNED, ids=[p[0] for p in PINNED])
def test_constants_the_ecselect_tests_straddle(name, value, test):
    _pinned(name, value, test)


def test_the_passes_over_the_entries_take_their_share_per_workgroup_and_the_scan_tile_is_the_product():
    src = _source()
    assert len(re.findall(r"k_sel_gather_a<<<nblk\(nnz_a, SEL_TPB \* SEL_ITEMS\), SEL_TPB, 0, st>>>", src)) == 1
    assert len(re.findall(r"const unsigned n_blocks = nblk\(nnz_n, SEL_TPB \* SEL_ITEMS\);", src)) == 1
    for k in ("k_sel_totals", "k_sel_nkeep", "k_sel_gather_n"):
        assert len(re.findall(r"%s<<<n_blocks, SEL_TPB, 0, st>>>" % k, src)) == 1, k
    assert len(re.findall(r"SCB = SCB_TPB \* SCB_ITEMS;", src)) == 1
    for name, value in SCAN:
        _pinned(name, value, "test_sizes_on_the_scans_stretch")
    assert (SCAN_TILE, SHARE) == (1024 * 16, 1024)
