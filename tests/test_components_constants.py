"""The constants ``test_gpu_ecclusters.py`` places its row lengths on, read from the kernel source (``alntools_amd/csrc/components.inc``): a
retune that moves one fails here, naming the test to rebuild around the new value (in the manner of ``test_count_constants.py``).  The GPU
tests import ``TPB``, ``CC_ITEMS`` and ``CC_WG_ITEMS`` from this file."""
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "alntools_amd", "csrc")
TPB, CC_ITEMS = 256, 4                      # threads per workgroup; non-zeros per thread of the hook pass ...
CC_WG_ITEMS = TPB * CC_ITEMS                # ... and per workgroup

PINNED = [
    ("components.inc", "u32", "CC_ITEMS", str(CC_ITEMS), "test_row_lengths_around_a_threads_and_a_workgroups_items"),
    ("components.inc", "u32", "CC_WG_ITEMS", "TPB * CC_ITEMS", "test_row_lengths_around_a_threads_and_a_workgroups_items"),
    ("ecb.hip", "int", "TPB", str(TPB), "test_row_lengths_around_a_threads_and_a_workgroups_items (TPB * CC_ITEMS = 1024)"),
]


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@pytest.mark.parametrize("file,ctype,name,value,test", PINNED, ids=[p[2] for p in PINNED])
def test_constants_the_ecclusters_tests_straddle(file, ctype, name, value, test):
    defs = re.findall(r"constexpr\s+%s\s+%s\s*=\s*([^;,]+);" % (ctype, name), _source(file))
    assert len(defs) == 1, "%d definitions of %s" % (len(defs), name)
    assert defs[0].strip() == value, ("%s is now %s (was %s): move the inputs of test_gpu_ecclusters.py::%s onto the new value"
                                      % (name, defs[0].strip(), value, test))


def test_the_hook_pass_is_launched_per_non_zero_with_these_constants():
    src = _source("components.inc")
    assert len(re.findall(r"k_cc_hook<(?:true|false)><<<nblk\(nnz, CC_WG_ITEMS\), TPB, 0, st>>>", src)) == 2
    assert "(u64)threadIdx.x * CC_ITEMS" in src and "blockIdx.x * (u64)CC_WG_ITEMS" in src
    # the sums are integer atomics, and nothing waits on the host for a fixed point
    assert "atomicAdd(reinterpret_cast<double" not in src and "unsafeAtomicAdd" not in src and "atomicAdd(double" not in src
    body = src[src.index('extern "C" int ecb_components_device'):src.index('extern "C" int ecb_components(')]
    assert not re.search(r"\b(while|for|do)\b", re.sub(r"//.*", "", body))
