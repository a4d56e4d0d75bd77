"""The constants ``test_gpu_count_alignments.py`` places its inputs on, read from the kernel source: a retune that moves one fails here,
naming the boundary test to rebuild around the new value (in the manner of ``test_threshold_constants.py``)."""
import os
import re

import pytest

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "alntools_amd", "csrc", "ecb.hip")

PINNED = [
    ("CA_LDS_BYTES", "80u << 10", "test_loci_on_the_window_and_sort_pass_limits (windows of 2048 / 2048 / 512 / 128 loci at 1 / 2 / 8 / 31 haplotypes)"),
    ("CA_TPB", "512", "test_non_zeros_on_the_workgroup_limits"),
    ("CA_CHUNK", "32768", "test_non_zeros_on_the_workgroup_limits (32 767 .. 32 769 and 65 537 non-zeros)"),
    ("CA_KEY_ITEMS", "4", "test_non_zeros_on_the_workgroup_limits (TPB * CA_KEY_ITEMS = 1024: 1023 .. 1025 non-zeros)"),
    ("CA_WIN_SHIFT", "40", "test_loci_on_the_window_and_sort_pass_limits (256 windows fill the digit at bit 40)"),
    ("GM_ITEMS", "4", "test_non_zeros_on_the_workgroup_limits"),
    ("TPB", "256", "test_non_zeros_on_the_workgroup_limits (TPB * CA_KEY_ITEMS = 1024)"),
]


def _source():
    with open(SRC) as f:
        return f.read()


@pytest.mark.parametrize("name,value,test", PINNED, ids=[p[0] for p in PINNED])
def test_constants_the_count_alignments_tests_straddle(name, value, test):
    defs = re.findall(r"constexpr\s+(?:u32|int)\s+(?:\w+\s*=\s*[^;,]+,\s*)*%s\s*=\s*([^;,]+)[;,]" % name, _source())
    assert len(defs) == 1, "%d definitions of %s" % (len(defs), name)
    assert defs[0].strip() == value, ("%s is now %s (was %s): move the inputs of test_gpu_count_alignments.py::%s onto the new value"
                                      % (name, defs[0].strip(), value, test))


def test_window_width_follows_the_lds_budget():
    """ca_window_bits: the largest power of two of loci whose 2 H + 1 eight-byte counters fit CA_LDS_BYTES -- the widths the tests use."""
    src = _source()
    assert len(re.findall(r"const u32 fit = CA_LDS_BYTES / 8u / \(2u \* n_haps \+ 1u\);", src)) == 1
    assert len(re.findall(r"return 31u - \(u32\)__builtin_clz\(fit\);", src)) == 1
    width = lambda h: 1 << ((80 << 10) // 8 // (2 * h + 1)).bit_length() - 1   # noqa: E731
    assert [width(h) for h in (1, 2, 8, 31)] == [2048, 2048, 512, 128]
