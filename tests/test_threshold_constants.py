"""The constants ``test_gpu_thresholds.py`` places its inputs on, read from the kernel sources: a retune that moves one fails here, naming
the boundary test to rebuild around the new value."""
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "alntools_amd", "csrc")

# (file, constant, expected definition, test in test_gpu_thresholds.py that sits on it)
PINNED = [
    ("k_stream.inc", "CMAX", "KS_SHORT ? 64 : 80", "test_reads_carrying_cmax_and_one_more_entries_over_a_tile_end, test_every_read_deferred"),
    ("k_stream.inc", "WMAXR", "KS_SHORT ? 128 : 64", "test_reads_of_a_whole_tile_and_tiles_of_many_reads"),
    ("ecb.hip", "RPL", "ECB_RPL", "test_reads_of_a_whole_tile_and_tiles_of_many_reads (WT = 64 * RPL)"),
    ("ecb.hip", "WT", "64 * RPL", "test_reads_of_a_whole_tile_and_tiles_of_many_reads, test_every_read_deferred"),
    ("ecb.hip", "SLOW_LDS", "4096", "test_k_slow_lds_limit"),
    ("ecb.hip", "INL", "5", "test_key_lengths_through_finalize_merge_adopt_and_ecb_merge"),
    ("ecb.hip", "RANKED_MAX", "16", "test_key_lengths_through_finalize_merge_adopt_and_ecb_merge"),
    ("ecb.hip", "BIG_LDS", "2048", "test_key_lengths_through_finalize_merge_adopt_and_ecb_merge, test_ecmerge_long_rows_one_and_31_haplotypes"),
    ("ecb.hip", "CVU_PIECE", "1536", "test_per_haplotype_csc_columns_on_the_piece_limits"),
    ("ecb.hip", "CVU_MAX", "3072", "test_per_haplotype_csc_columns_on_the_piece_limits"),
    ("ecb.hip", "CVU_TSZ", "4096", "test_per_haplotype_csc_columns_on_the_piece_limits (a piece of CVU_MAX fills 3/4 of it)"),
    ("ecb.hip", "QSTRIPES", "64", "test_every_read_deferred"),
    ("ecb.hip", "MSF_LDS_CELLS", "8192", "test_gpu_multisample.py::test_cell_counts_on_the_lds_limit_and_the_radix_tile"),
    ("ecb.hip", "MSF_SMALL", "256", "test_gpu_multisample.py::test_ecs_on_the_thread_workgroup_and_grid_limits_and_every_meta_edge"),
    ("ecb.hip", "MSF_GIANT", "1u << 15", "test_gpu_multisample.py::test_ecs_on_the_thread_workgroup_and_grid_limits_and_every_meta_edge"),
]


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@pytest.mark.parametrize("fname,name,value,test", PINNED, ids=[p[1] for p in PINNED])
def test_constants_the_boundary_tests_straddle(fname, name, value, test):
    defs = re.findall(r"constexpr\s+(?:u32|int)\s+%s\s*=\s*([^;]+);" % name, _source(fname))
    assert len(defs) == 1, "%s: %d definitions of %s" % (fname, len(defs), name)
    where = test if "::" in test else "test_gpu_thresholds.py::" + test
    assert defs[0].strip() == value, ("%s is now %s in %s (was %s): move the inputs of %s onto the new value"
                                      % (name, defs[0].strip(), fname, value, where))


def test_records_per_lane_default():
    """WT = 64 * ECB_RPL records: ECB_RPL defaults to 8 (512-record tiles), and k_stream insists on 512."""
    assert re.search(r"#ifndef ECB_RPL\s*\n#define ECB_RPL 8\b", _source("ecb.hip"))
    assert "static_assert(WT == 512" in _source("k_stream.inc")


def test_cell_bits():
    """22 bits of cell id under 10 of file in the meta word: ecb.h, the host that packs it, and test_gpu_multisample.py's top cell
    2^22 - 1 in file 1023 (meta 0xFFFFFFFF)."""
    with open(os.path.join(CSRC, "..", "..", "include", "ecb.h")) as f:
        assert re.findall(r"#define ECB_CELL_BITS\s+(\d+)", f.read()) == ["22"]
    with open(os.path.join(CSRC, "..", "bam_utils_multisample.py")) as f:
        assert re.findall(r"^CELL_BITS\s*=\s*(\d+)", f.read(), re.M) == ["22"]
    assert re.search(r"constexpr u32 MS_FILE_BITS = 32 - ECB_CELL_BITS;", _source("ecb.hip"))
