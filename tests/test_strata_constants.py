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
    atomics = re.findall(r"atomic\w+\(", src)
    assert atomics.count("atomicMin(") == 4 and len(atomics) == 5   # the crossing reads' words and first passing records to their slots, and ...
    assert src.count("atomicAdd(") == 1 and "k_strata_sum" in src   # the four counts: integers, added up per 16 x 256 waves, never per wave of records
    # the only places a slot is named: by the wave's own number, or by a record's position (strata_read_start) over the span
    assert re.findall(r"\b[ht]s = \(u32\)([^;]+);", src) == ["(strata_read_start(rid, rid[0], base, a.rel[0]) / STRATA_WAVE_RECS)", "w"]
    # the lowest offender: the three reasons are the shared step rule's, one call of it, its verdict to the shared word
    assert src.count("tuple_step(prev, a.id[q], a.pass[q])") == src.count("tuple_step(") == 1
    assert src.count("if (why) offender(err, i + q, why);") == src.count("offender(") - src.count("refuse_offender(") == 1


def test_the_lowest_offender_and_the_step_rule_are_defined_once_in_the_tree():
    tree = "".join(_source(f) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".inc", ".h")))
    assert len(re.findall(r"\bvoid offender\(", tree)) == 1 and len(re.findall(r"\bu32 tuple_step\(", tree)) == 1
    assert len(re.findall(r"atomicMin\([^;]*<< 8 \| reason", tree)) == 1
    assert len(re.findall(r"\bconst char\* tuple_reason\(", tree)) == 1 and len(re.findall(r"TUPLE_R_FALLS = 1, TUPLE_R_JUMPS, TUPLE_R_FILTERED", tree)) == 1
    for text in ("read_id falls", "read_id steps by more than 1", "read_id steps on a record that does not pass the filter"):
        assert tree.count('"%s"' % text) == 1, text
