"""The spans ``test_gpu_best_strata.py`` places its sizes on -- records per lane, per wave, per workgroup -- read from the kernel source
(``alntools_amd/csrc/strata.inc``, ``ecb.hip``): a retune that moves one fails here, naming the tests to rebuild around the new value (in
the manner of ``test_bus_correct_constants.py``).  The GPU tests import L, W and G from this file."""
import os
import re

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CSRC = os.path.join(ROOT, "alntools_amd", "csrc")
TPB = 256                      # threads per workgroup: four waves
L = 4                          # STRATA_LANE_RECS: records per lane, one 16-byte vector of each stream
W = 64 * L                     # STRATA_WAVE_RECS: records per wave -- what a wave settles by shuffles
G = (TPB // 64) * W            # STRATA_WG_RECS: records per workgroup

PINNED = [
    ("strata.inc", "u32", "STRATA_LANE_RECS", "4", "test_tiny_streams, test_short_reads_at_every_offset"),
    ("strata.inc", "u32", "STRATA_WAVE_RECS", "64 * STRATA_LANE_RECS", "test_a_read_boundary_around_every_span, test_long_reads"),
    ("strata.inc", "u32", "STRATA_WG_RECS", "(TPB / 64) * STRATA_WAVE_RECS", "test_a_read_boundary_around_every_span, test_long_reads"),
    ("ecb.hip", "int", "TPB", str(TPB), "test_a_read_boundary_around_every_span"),
]


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@pytest.mark.parametrize("file,ctype,name,value,test", PINNED, ids=[p[2] for p in PINNED])
def test_constants_the_strata_tests_straddle(file, ctype, name, value, test):
    defs = re.findall(r"constexpr\s+%s\s+%s\s*=\s*([^;]+);" % (ctype, name), _source(file))
    assert len(defs) == 1, "%d definitions of %s" % (len(defs), name)
    assert defs[0].split("//")[0].strip() == value, ("%s is now %s (was %s): move the inputs of test_gpu_best_strata.py::%s onto the new value"
                                                     % (name, defs[0].strip(), value, test))
    assert (L, W, G) == (4, 256, 1024)


def test_the_spans_are_what_the_launches_use_and_there_is_one_path():
    src = re.sub(r"//.*", "", _source("strata.inc"))
    # both kernels are launched a workgroup per STRATA_WG_RECS records, whatever n is: no switch on the input's size
    assert src.count("<<<nblk(n, STRATA_WG_RECS), TPB, 0, st>>>") == 2 and src.count("<<<") == 3      # (the third adds the waves' counts up)
    assert "const uint4 q = *reinterpret_cast<const uint4*>(p + i);" in src and "__shfl_up(" in src and "__ballot(" in src


def test_no_index_comes_from_a_read_id_and_nothing_is_placed_by_an_atomic():
    src = re.sub(r"//.*", "", _source("strata.inc"))
    assert set(re.findall(r"atomic\w+\(", src)) == {"atomicMin(", "atomicAdd("}
    assert src.count("atomicAdd(") == 1 and "k_strata_sum" in src   # the four counts: integers, added up per 16 x 256 waves, never per wave of records
    # the only places a slot is named: by the wave's own number, or by a record's position (strata_read_start) over the span
    assert re.findall(r"\b[ht]s = \(u32\)([^;]+);", src) == ["(strata_read_start(rid, rid[0], base, a.rel[0]) / STRATA_WAVE_RECS)", "w"]
    assert src.count("bus_err(err, i + q, ") == 2                    # the lowest offender: three reasons, two call sites
