"""The constants ``test_gpu_ecdownsample.py`` places its sizes on -- the largest sample one workgroup thins, the reads of a thread, a wave
and a workgroup of the passes over the large samples (``alntools_amd/csrc/downsample.inc``) -- read from the kernel source: a retune that
moves one fails here, naming the tests to rebuild around the new value (in the manner of ``test_umi_constants.py``).  The GPU tests import
SMALL, THREAD, WAVE and WG from this file."""
import os
import re

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CSRC = os.path.join(ROOT, "alntools_amd", "csrc")
TPB = 256                      # threads per workgroup: four waves
SMALL = 2048                   # DS_SMALL: a sample of at most this many reads is one workgroup's
THREAD = 16                    # DS_THREAD_READS: consecutive reads per thread of a pass over the large samples
WAVE = 64 * THREAD             # DS_WAVE_READS
WG = TPB * THREAD              # DS_WG_READS: a stretch

PINNED = [
    ("downsample.inc", "u32", "DS_SMALL", str(SMALL), "test_sizes_of_a_sample, test_the_word_boundary_of_the_key (redo the search: SMALL_CASE)"),
    ("downsample.inc", "u32", "DS_SMALL_READS", "DS_SMALL / TPB", "test_sizes_of_a_sample"),
    ("downsample.inc", "u32", "DS_THREAD_READS", str(THREAD), "test_boundaries_on_either_side_of_every_stretch"),
    ("downsample.inc", "u32", "DS_WAVE_READS", "64 * DS_THREAD_READS", "test_boundaries_on_either_side_of_every_stretch"),
    ("downsample.inc", "u32", "DS_WG_READS", "TPB * DS_THREAD_READS", "test_sizes_of_a_sample, test_boundaries_on_either_side_of_every_stretch"),
    ("downsample.inc", "u32", "DS_BINS", "256", "test_the_word_boundary_of_the_key"),
    ("downsample.inc", "u32", "DS_DIGITS", "16", "test_the_word_boundary_of_the_key"),
    ("ecb.hip", "int", "TPB", str(TPB), "test_boundaries_on_either_side_of_every_stretch"),
]


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@pytest.mark.parametrize("file,ctype,name,value,test", PINNED, ids=[p[2] for p in PINNED])
def test_constants_the_downsample_tests_straddle(file, ctype, name, value, test):
    defs = re.findall(r"constexpr\s+%s\s+%s\s*=\s*([^;]+);" % (ctype, name), _source(file))
    assert len(defs) == 1, "%d definitions of %s" % (len(defs), name)
    assert defs[0].split("//")[0].strip() == value, ("%s is now %s (was %s): move the inputs of test_gpu_ecdownsample.py::%s onto the new value"
                                                     % (name, defs[0].strip(), value, test))
    assert (SMALL, THREAD, WAVE, WG) == (2048, 16, 1024, 4096)


def test_the_relations_the_kernels_rely_on_are_asserted_and_the_header_names_the_sizes():
    src = _source("downsample.inc")
    for text in ("DS_BINS == (u32)TPB", "DS_SMALL == DS_SMALL_READS * (u32)TPB", "DS_SMALL < (1u << 16)", "DS_WG_READS == 4u * DS_WAVE_READS",
                 "8u * DS_DIGITS == 128u"):
        assert "static_assert(" + text in src, text
    hdr = open(os.path.join(ROOT, "include", "ecb_downsample.h")).read()
    assert "M_s above %d" % SMALL in hdr and "stretches of %d reads" % WG in hdr      # the header states the further limit in these sizes


def test_no_key_is_stored_no_float_atomic_and_no_assembly():
    src = re.sub(r"//.*", "", _source("downsample.inc"))
    assert "asm" not in src and "hipMalloc" not in src and "radix_sort_pairs64" not in src
    assert "atomicAdd(reinterpret_cast<double" not in src and "unsafeAtomicAdd" not in src and "float" not in src
    # every key is made where it is looked at: the three kernels that look at keys call ds_key, and no array of keys leaves a kernel
    assert src.count("ds_key(seed, ") == 3 and "DsKey*" not in src
    # the passes over the large samples are launched a workgroup per stretch, whatever the entries' counts are
    assert src.count("<<<(unsigned)n_stretches, TPB, 0, st>>>") == 2 and src.count("<<<(unsigned)n_large, TPB, 0, st>>>") == 1
    main = _source("ecb.hip")
    assert main.index('#include "umi.inc"') < main.index('#include "ds_key.h"') < main.index('#include "downsample.inc"')
    assert len(re.findall(r'^#include "downsample\.inc"', main, re.M)) == 1
