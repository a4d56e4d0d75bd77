"""The spans ``test_gpu_collapse_umis.py`` places its sizes on -- records per lane, per wave, per workgroup of ``csrc/umi.inc``, the
sort's tile and the scan's stretch of ``ecb.hip`` -- read from the kernel source: a retune that moves one fails here, naming the tests to
rebuild around the new value (in the manner of ``test_strata_constants.py``).  The GPU tests import L, W, G, TILE and STRETCH from this
file."""
import os
import re

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CSRC = os.path.join(ROOT, "alntools_amd", "csrc")
TPB = 256                      # threads per workgroup: four waves
L = 1                          # UMI_LANE_RECS: every kernel of umi.inc is a map, one element per thread
W = 64 * L                     # UMI_WAVE_RECS
G = (TPB // 64) * W            # UMI_WG_RECS
TILE = 4096                    # RS_TILE: pairs per workgroup of a sort pass
STRETCH = 1024 * 16            # SCB: values per workgroup of a scan

PINNED = [
    ("umi.inc", "u32", "UMI_LANE_RECS", "1", "test_tiny_streams"),
    ("umi.inc", "u32", "UMI_WAVE_RECS", "64 * UMI_LANE_RECS", "test_molecule_sizes, test_edges"),
    ("umi.inc", "u32", "UMI_WG_RECS", "(TPB / 64) * UMI_WAVE_RECS", "test_molecule_sizes, test_edges"),
    ("umi.inc", "u32", "UMI_HAP_BITS", "5", "test_the_largest_locus_and_haplotype"),
    ("umi.inc", "u32", "UMI_LOC_BITS", "26", "test_the_largest_locus_and_haplotype"),
    ("umi.inc", "u32", "UMI_MM_BITS", "30", "test_the_largest_locus_and_haplotype"),
    ("ecb.hip", "int", "TPB", str(TPB), "test_edges"),
    ("ecb.hip", "u32", "MAX_LOCI", "(1u << 26) - 2u", "test_the_largest_locus_and_haplotype"),
]


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@pytest.mark.parametrize("file,ctype,name,value,test", PINNED, ids=[p[2] for p in PINNED])
def test_constants_the_umi_tests_straddle(file, ctype, name, value, test):
    defs = re.findall(r"constexpr\s+%s\s+%s\s*=\s*([^;]+);" % (ctype, name), _source(file))
    assert len(defs) == 1, "%d definitions of %s" % (len(defs), name)
    assert defs[0].split("//")[0].strip() == value, ("%s is now %s (was %s): move the inputs of test_gpu_collapse_umis.py::%s onto the new value"
                                                     % (name, defs[0].strip(), value, test))
    assert (L, W, G) == (1, 64, 256)


def test_the_sort_tile_and_the_scan_stretch():
    src = _source("ecb.hip")
    assert re.search(r"constexpr int RS_TPB = ECB_RS_TPB, RS_TILE = (\d+),", src).group(1) == str(TILE)
    m = re.search(r"constexpr int SCB_TPB = (\d+), SCB_ITEMS = (\d+), SCB = SCB_TPB \* SCB_ITEMS;", src)
    assert int(m.group(1)) * int(m.group(2)) == STRETCH


def test_one_path_whatever_the_size_and_nothing_placed_by_an_atomic():
    src = re.sub(r"//.*", "", _source("umi.inc"))
    # every kernel but the one-thread search is launched a workgroup per UMI_WG_RECS elements: no switch on a size, no "long run" path
    launches = re.findall(r"<<<(\w+(?:\([^)]*\))?), (\w+), 0, st>>>", src)
    assert len(launches) == src.count("<<<") == 16 and all(tpb in ("TPB", "64") for _, tpb in launches)
    assert [g for g, tpb in launches if tpb == "64"] == ["1"]
    assert all(g.startswith("grid_") or g == "nblk(n_runs, UMI_WG_RECS)" for g, tpb in launches if tpb == "TPB")
    assert set(re.findall(r"= nblk\((\w+), UMI_WG_RECS\);", src)) == {"n", "R", "m", "n_runs"}
    # the only atomic is the lowest offender's minimum (ecb.hip's offender), read by refusals alone; no float atomics; one sort implementation
    assert re.findall(r"atomic\w+\(", src) == [] and src.count("offender(err, i, ") == src.count("offender(") - src.count("refuse_offender(") == 3
    assert src.count("tuple_step(i ? rid[i - 1] : id, id, ok)") == src.count("tuple_step(") == 1       # the step rule's three reasons; locus; haplotype
    assert "UMI_R_LOCUS == 4 && UMI_R_HAP == 5" in src and "default: return tuple_reason(r);" in src
    assert src.count("radix_sort_pairs64(") == 2 and "k_rs_" not in src and "hipMalloc" not in src
    # the second sort is behind the test for a molecule of several reads
    assert src.index("if (n_multi) {") < src.index("radix_sort_pairs64(st, s2")
