"""The constants ``test_gpu_buscorrect.py`` places its sizes on, read from the kernel source (``alntools_amd/csrc/bus_correct.inc``,
``ecb.hip``): a retune that moves one fails here, naming the test to rebuild around the new value (in the manner of
``test_bus_constants.py``).  The GPU tests import the values and :func:`dir_bits` from this file."""
import os
import re

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CSRC = os.path.join(ROOT, "alntools_amd", "csrc")
TPB = 256                      # threads per workgroup of the maps; four misses (waves) per workgroup of the neighbour search
SCB = 1024 * 16                # values per workgroup of a scan
BUSC_BISECT_LEN = 16           # a bucket up to this long is read whole, a longer one bisected
BUSC_BUCKET_AVG = 4            # the directory's sizing rule: the fewest bits with n_white <= BUSC_BUCKET_AVG << bits ...
BUSC_DIR_MAX_BITS = 24         # ... at most this many, and at most 2 x bclen
BUSC_LANES = 64                # lanes per miss: a wave


def dir_bits(n_white, bclen):
    """The sizing rule as ``bus_correct.inc``'s header states it."""
    b = 0
    while b < BUSC_DIR_MAX_BITS and b < 2 * bclen and (BUSC_BUCKET_AVG << b) < n_white:
        b += 1
    return b


PINNED = [
    ("bus_correct.inc", "u32", "BUSC_BISECT_LEN", str(BUSC_BISECT_LEN), "test_one_bucket_below_at_and_above_the_bisection_length"),
    ("bus_correct.inc", "u32", "BUSC_BUCKET_AVG", str(BUSC_BUCKET_AVG), "test_whitelists_on_both_sides_of_every_directory_size"),
    ("bus_correct.inc", "u32", "BUSC_DIR_MAX_BITS", str(BUSC_DIR_MAX_BITS), "test_whitelists_on_both_sides_of_every_directory_size"),
    ("bus_correct.inc", "u32", "BUSC_LANES", str(BUSC_LANES), "test_barcode_lengths_and_bit_edges (63 and 66 neighbours) and test_sizes"),
    ("ecb.hip", "int", "TPB", str(TPB), "test_sizes"),
    ("ecb.hip", "int", "SCB_TPB", "1024, SCB_ITEMS = 16, SCB = SCB_TPB * SCB_ITEMS", "test_sizes"),
]


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@pytest.mark.parametrize("file,ctype,name,value,test", PINNED, ids=[p[2] for p in PINNED])
def test_constants_the_buscorrect_tests_straddle(file, ctype, name, value, test):
    defs = re.findall(r"constexpr\s+%s\s+%s\s*=\s*([^;]+);" % (ctype, name), _source(file))
    assert len(defs) == 1, "%d definitions of %s" % (len(defs), name)
    assert defs[0].split("//")[0].strip() == value, ("%s is now %s (was %s): move the inputs of test_gpu_buscorrect.py::%s onto the new value"
                                                     % (name, defs[0].strip(), value, test))


def test_the_directorys_sizing_rule_and_the_path_switch_are_named():
    src = re.sub(r"//.*", "", _source("bus_correct.inc"))
    assert "while (b < BUSC_DIR_MAX_BITS && b < 2 * bclen && ((u64)BUSC_BUCKET_AVG << b) < n_white) ++b;" in src, \
        "the sizing rule moved: dir_bits above and test_gpu_buscorrect.py::test_whitelists_on_both_sides_of_every_directory_size"
    assert src.count("hi - lo <= BUSC_BISECT_LEN") == 1, "test_gpu_buscorrect.py::test_one_bucket_below_at_and_above_the_bisection_length"
    # one lookup for the exact pass and the neighbour search, and a wave per miss
    assert src.count("busc_has(t, ") == 2 and "TPB / BUSC_LANES" in src and "__ballot(hit)" in src
    assert [dir_bits(n, 16) for n in (1, 4, 5, 8, 9, 6800000, 1 << 30)] == [0, 0, 1, 1, 2, 21, 24] and dir_bits(1000, 1) == 2 and dir_bits(17, 32) == 3


def test_nothing_is_placed_by_an_atomic():
    src = re.sub(r"//.*", "", _source("bus_correct.inc"))
    assert re.findall(r"atomic\w+\(", src) == []                   # none of its own: only ecb.hip's offender, the lowest offender's minimum
    assert src.count("offender(err, ") == src.count("offender(") - src.count("refuse_offender(") == 3      # two reasons for an entry, one for a record
