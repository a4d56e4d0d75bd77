"""The constants ``test_gpu_bus2ec.py`` places its sizes on, read from the kernel source (``alntools_amd/csrc/bus.inc``, ``ecb.hip``) and the
header: a retune that moves one fails here, naming the test to rebuild around the new value (in the manner of
``test_components_constants.py``).  The GPU tests import the values from this file."""
import os
import re

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CSRC = os.path.join(ROOT, "alntools_amd", "csrc")
TPB = 256                      # threads per workgroup of the run-head kernels: a molecule's records on both sides of a thread's neighbour in another workgroup
RS_TILE = 4096                 # keys per workgroup of a sort pass
SCB = 1024 * 16                # values per workgroup of a scan
BUS_WAVE_WORK = 128            # candidates x (k - 1) from which an intersection is a wave's
BUS_MERGE_LEN = 8              # a line up to this long is walked, a longer one bisected
MAX_UMILEN = 16

PINNED = [
    ("bus.inc", "u32", "BUS_WAVE_WORK", str(BUS_WAVE_WORK), "test_intersections_on_both_sides_of_every_path_switch and test_molecules_of_k_ecs"),
    ("bus.inc", "u32", "BUS_MERGE_LEN", str(BUS_MERGE_LEN), "test_intersections_on_both_sides_of_every_path_switch"),
    ("bus.inc", "u32", "BUS_MAX_UMILEN", "ECB_BUS_MAX_UMILEN", "test_umi_zero_and_all_ones"),
    ("ecb.hip", "int", "TPB", str(TPB), "test_molecules_across_a_thread_workgroup_and_tile_edge"),
    ("ecb.hip", "int", "SCB_TPB", "1024, SCB_ITEMS = 16, SCB = SCB_TPB * SCB_ITEMS", "test_molecules_across_a_thread_workgroup_and_tile_edge"),
]


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@pytest.mark.parametrize("file,ctype,name,value,test", PINNED, ids=[p[2] for p in PINNED])
def test_constants_the_bus2ec_tests_straddle(file, ctype, name, value, test):
    defs = re.findall(r"constexpr\s+%s\s+%s\s*=\s*([^;]+);" % (ctype, name), _source(file))
    assert len(defs) == 1, "%d definitions of %s" % (len(defs), name)
    assert defs[0].split("//")[0].strip() == value, ("%s is now %s (was %s): move the inputs of test_gpu_bus2ec.py::%s onto the new value"
                                                     % (name, defs[0].strip(), value, test))


def test_the_sort_tile_and_the_umi_limit():
    assert re.search(r"constexpr int RS_TPB = ECB_RS_TPB, RS_TILE = %d," % RS_TILE, _source("ecb.hip")), "RS_TILE moved: test_molecules_across_a_thread_workgroup_and_tile_edge"
    with open(os.path.join(ROOT, "include", "ecb_bus.h")) as f:
        assert re.search(r"#define ECB_BUS_MAX_UMILEN %du\b" % MAX_UMILEN, f.read()), "the UMI limit moved: test_umi_zero_and_all_ones"
    from alntools_amd import ecb_bus
    assert ecb_bus.MAX_UMILEN == MAX_UMILEN and ecb_bus.NO_UMI == 1


def test_no_path_switch_is_an_unnamed_literal_and_nothing_is_placed_by_an_atomic():
    src = re.sub(r"//.*", "", _source("bus.inc"))
    assert "(u64)clen * (k - 1u) >= BUS_WAVE_WORK" in src and "hi - lo <= BUS_MERGE_LEN" in src
    # both intersection kernels take their path from the one predicate
    assert src.count("bus_wave_path(len, b - a)") == 2
    # the only atomics: the error bits, and the lowest offender's minimum through ecb.hip's offender (five breaches of a line, three of a record)
    assert re.findall(r"atomic\w+\(", src) == ["atomicOr("] * 2
    assert src.count("offender(err, ") == src.count("offender(") - src.count("refuse_offender(") == 8
