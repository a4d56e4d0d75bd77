"""The constants ``test_gpu_thresholds.py``, ``test_gpu_multisample.py`` and ``test_gpu_counting.py`` (with ``counting_streams.py``, which
restates the counting pass's arithmetic) place their inputs on, read from the kernel sources: a retune that moves one fails here, naming
the boundary test to rebuild around the new value."""
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "alntools_amd", "csrc")

# (file, constant, expected definition, test that sits on it: in test_gpu_thresholds.py unless it names its file)
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
    ("ecb.hip", "BIN_BITS", "14", "test_gpu_counting.py::test_slots_per_range_and_table_size (test_counting_streams.py::test_ranges_per_table_size_and_knob)"),
    ("ecb.hip", "MIN_BIN_BITS", "11", "test_gpu_counting.py::test_slots_per_range_and_table_size (tables of 2^10 and 2^16 slots)"),
    ("ecb.hip", "MAX_BIN_BITS", "15", "test_gpu_counting.py::test_slots_per_range_and_table_size (the table of 2^28 slots, ECB_BIN_BITS = 15)"),
    ("ecb.hip", "MAX_BUCKETS", "8192", "test_gpu_counting.py::test_slots_per_range_and_table_size (tables of 2^24, 2^27 and 2^28 slots)"),
    ("ecb.hip", "STAGE_MAX_BUCKETS", "4096", "test_gpu_counting.py::test_slots_per_range_and_table_size (4096 and 8192 ranges at 2^24 and 2^27 slots)"),
    ("ecb.hip", "TPB_PART", "1024", "test_gpu_counting.py::test_slots_per_range_and_table_size (1024 / 2048 / 4096 ranges: 1, 2, 4 per thread of the staged scatter)"),
    ("ecb.hip", "STAGE", "8 * TPB_PART", "test_gpu_counting.py::test_read_counts_on_the_partition_edges (8191 .. 8193 reads)"),
    ("ecb.hip", "PART_G", "512", "test_gpu_counting.py::test_read_counts_on_the_partition_edges (2 097 151 .. 2 097 153 reads)"),
    ("ecb.hip", "BM_LINE", "16", "test_gpu_counting.py::test_first_appearances_on_the_bitmap_line_ends (reads 510 .. 513, 16 383, 16 384)"),
    ("ecb.hip", "SCB_TPB", "1024", "test_gpu_counting.py::test_ranking_across_the_first_stretch_of_the_scan (SCB_TPB * SCB_ITEMS lines of 512 reads = 8 388 608 reads)"),
    ("ecb.hip", "SCB_ITEMS", "16", "test_gpu_counting.py::test_ranking_across_the_first_stretch_of_the_scan"),
]


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@pytest.mark.parametrize("fname,name,value,test", PINNED, ids=[p[1] for p in PINNED])
def test_constants_the_boundary_tests_straddle(fname, name, value, test):
    # (one declaration may define several: `constexpr int A = 1, B = 2;`)
    defs = re.findall(r"constexpr\s+(?:u32|int)\s+(?:\w+\s*=\s*[^;,]+,\s*)*%s\s*=\s*([^;,]+)[;,]" % name, _source(fname))
    assert len(defs) == 1, "%s: %d definitions of %s" % (fname, len(defs), name)
    where = test if "::" in test else "test_gpu_thresholds.py::" + test
    assert defs[0].strip() == value, ("%s is now %s in %s (was %s): move the inputs of %s onto the new value"
                                      % (name, defs[0].strip(), fname, value, where))


# lines of ecb.hip that hold a threshold no constant names: (pattern, what it is, test that sits on it)
PINNED_LINES = [
    (r"const u32 piece = std::max<u32>\(32768u, 2u \* \(u32\)\(\(R \+ nb - 1\) / nb\)\);", "a piece of a cut range: at least 32768 reads, twice the average range",
     "test_gpu_counting.py::test_cut_ranges_through_every_sink"),
    (r"const bool cut = len > piece \+ piece / 2;", "a range is cut above 1.5 pieces", "test_gpu_counting.py::test_cut_ranges_through_every_sink"),
    (r"const u32 G = \(u32\)std::min<u64>\(PART_G, \(R \+ 4095\) / 4096\);", "4096 reads per workgroup of the partition passes",
     "test_gpu_counting.py::test_read_counts_on_the_partition_edges"),
    (r"part_per\(u64 n_reads, u64 G\) \{ return \(\(\(n_reads \+ G - 1\) / G\) \+ 3ull\) & ~3ull; \}", "a workgroup's reads, rounded up to 4",
     "test_gpu_counting.py::test_read_counts_on_the_partition_edges"),
    (r"if \(__popcll\(m\) >= 8\) \{", "eight equal lanes of a wave are added once", "test_gpu_counting.py::test_runs_of_one_slot_in_a_wave"),
]


@pytest.mark.parametrize("pattern,what,test", PINNED_LINES, ids=[p[1] for p in PINNED_LINES])
def test_unnamed_thresholds_of_the_counting_pass(pattern, what, test):
    assert len(re.findall(pattern, _source("ecb.hip"))) == 1, "%s: the line changed -- rebuild %s (and counting_streams.py) around it" % (what, test)


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
