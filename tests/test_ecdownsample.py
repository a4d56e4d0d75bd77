"""ecdownsample without a GPU: the checker (``tests/downsample_checker.py``) held to a brute-force sort of Python tuples and to Random123's
known answers, the key file (``alntools_amd/csrc/ds_key.h``) compiled as plain C++ against the checker's Python integers -- all sixteen
digits, and a radix select on its helpers as the kernels run it --, the moments of the rule against the hypergeometric law, the ABI's
header against the module's symbols, the targets of ``-f`` and ``--equalize``, and the command's wiring, refusals and exit status with the
device calls replaced by the checkers.  The GPU side is ``tests/test_gpu_ecdownsample.py``."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from alntools_amd import bin_utils, ecb, ecb_downsample as ed

import boot_checker as bc
import downsample_checker as dc
from test_ecboot import KAT
from test_ecselect import _fake_select

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "alntools_amd", "csrc")


def _bytes(p):
    with open(p, "rb") as f:
        return f.read()


@pytest.fixture(autouse=True)
def _logger_level_as_it_was():
    import logging
    log = logging.getLogger("alntools.utils")
    level = log.level
    yield
    log.setLevel(level)


# ---- 1. the checker ---------------------------------------------------------------------------------------------------------------------------
#         counts of the column's entries      sample  n   seed
DOZEN = [((1,), 0, 0, 0), ((1,), 0, 1, 0), ((2,), 0, 1, 0), ((1, 1), 1, 1, 0), ((3, 0, 2), 0, 2, 1), ((0, 0, 4, 0), 7, 3, 1), ((5, 5), 2, 9, 2),
         ((5, 5), 2, 10, 2), ((5, 5), 2, 11, 2), ((5, 5), 2, -1, 2), ((1, 2, 3, 4, 5, 6), 3, 7, 1 << 63), ((9, 1, 0, 1, 9), (1 << 32) - 1, 10, 12345),
         ((0, 0), 4, 0, 0), ((7,), 5, 3, (1 << 64) - 1)]


@pytest.mark.parametrize("counts,s,n,seed", DOZEN, ids=["%s-s%d-n%d" % ("_".join(map(str, c[0])), c[1], c[2]) for c in DOZEN])
def test_the_checker_against_a_sort_of_python_tuples(counts, s, n, seed):
    got = dc.thin_column(counts, s, n, seed)
    assert got.tolist() == dc.brute_column(counts, s, n, seed)
    M = sum(counts)
    assert int(got.sum()) == (M if n < 0 or n >= M else n) and all(0 <= g <= c for g, c in zip(got, counts))


def test_a_samples_draw_is_its_own_and_the_whole_call_is_the_columns_side_by_side():
    ptr, ec, cnt = [0, 3, 3, 5, 9], [0, 2, 2, 1, 0, 3, 2, 1, 0], [4, 0, 6, 1, 1, 2, 2, 5, 0]
    out, tin, tout = dc.downsample(ptr, ec, cnt, 4, [5, 3, 1, -1], seed=9)
    assert tin.tolist() == [10, 0, 2, 9] and tout.tolist() == [5, 0, 1, 9] and out.dtype == np.int32
    assert out[:3].tolist() == dc.thin_column([4, 0, 6], 0, 5, 9).tolist() and out[5:].tolist() == [2, 2, 5, 0]
    alone = dc.downsample(ptr, ec, cnt, 4, [5, -1, -1, 0], seed=9)[0]
    assert alone[:3].tolist() == out[:3].tolist() and alone[5:].tolist() == [0, 0, 0, 0]      # whatever the other targets are
    assert dc.breach([0, 2, 1, 3], [0, 1, 2], [1, 1, 1], 3) == "column pointers" and dc.breach([0, 3], [0, 1, 3], [1, 1, 1], 3).startswith("an EC index")
    assert dc.breach([0, 3], [0, 1, 2], [1, -1, 1], 3) == "a negative count" and dc.breach([0], [], [], 0) is None


@pytest.mark.parametrize("counter,key,want", KAT, ids=["zeros", "ones", "pi"])
def test_the_key_is_random123s_philox_at_the_headers_counter(counter, key, want):
    assert " ".join("%08x" % int(v) for v in bc.philox(counter, key)) == want
    # counter (r, 0, s, 1), key (seed's low word, seed's high word); o3 the most significant word
    seed, s, r = key[1] << 32 | key[0], counter[2], counter[0]
    o = [int(v) for v in bc.philox((r, 0, s, 1), key)]
    assert dc.key(seed, s, r) == o[3] << 96 | o[2] << 64 | o[1] << 32 | o[0]
    assert [dc.digit(dc.key(seed, s, r), d) for d in range(16)] == [(o[3 - d // 4] >> (8 * (3 - d % 4))) & 255 for d in range(16)]
    if counter == (0, 0, 0, 0):                                  # the fourth counter word keeps the stream apart from ecboot's
        assert dc.key(0, 0, 0) != int("9b00dbd8" "bc57ac4c" "e169c58d" "6627e8d5", 16)


# ---- 2. the key file as plain C++ -------------------------------------------------------------------------------------------------------------
MAIN = r"""
#include <cinttypes>
#include <cstdio>
#include <vector>
#include "ds_key.h"
// "k seed s r": the key's four words (o3 first) and its sixteen digits.  "s seed s M n": a radix select on the file's helpers as the
// kernels run it (histogram of digit d over the reads that match the prefix, the bin of the n-th, resolved or deeper), then the reads
// whose first depth + 1 digits are at most the prefix's; prints depth and the reads that stay.
int main() {
    char what;
    unsigned long long seed, s, a, b;
    while (std::scanf(" %c %llu %llu %llu %llu", &what, &seed, &s, &a, &b) == 5) {
        if (what == 'k') {
            const DsKey k = ds_key((uint64_t)seed, (uint32_t)s, (uint32_t)a);
            std::printf("%" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32, k.v[3], k.v[2], k.v[1], k.v[0]);
            for (uint32_t d = 0; d < 16; ++d) std::printf(" %" PRIu32, ds_digit(k, d));
            std::printf("\n");
            continue;
        }
        const uint32_t M = (uint32_t)a;
        uint32_t need = (uint32_t)b, depth = 0;
        DsKey pfx = DsKey();
        for (uint32_t d = 0; d < 16; ++d) {
            std::vector<uint32_t> h(256, 0);
            for (uint32_t r = 0; r < M; ++r) { const DsKey k = ds_key((uint64_t)seed, (uint32_t)s, r); if (ds_match(k, pfx, d)) ++h[ds_digit(k, d)]; }
            uint32_t bin = 0, below = 0;
            while (below + h[bin] < need) below += h[bin++];
            ds_set_digit(pfx, d, bin);
            depth = d;
            if (need == below + h[bin]) break;
            need -= below;
        }
        std::printf("%" PRIu32, depth);
        for (uint32_t r = 0; r < M; ++r) if (ds_at_most(ds_key((uint64_t)seed, (uint32_t)s, r), pfx, depth + 1)) std::printf(" %" PRIu32, r);
        std::printf("\n");
    }
    return 0;
}
"""
#: (seed, s, M, n) whose select goes into the key's second word: two reads share o3 and n puts the threshold between them (found with the
#: checker; test_gpu_ecdownsample.py runs the same ones on the device and re-checks the property)
SECOND_WORD = [(0, 1147, 2048, 518), (0, 2187, 2048, 1507), (0, 0, 1 << 17, 36672)]


def _host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    (tmp_path / "main.cc").write_text(MAIN)
    exe = str(tmp_path / "dskey")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", exe, str(tmp_path / "main.cc")])
    return lambda lines: subprocess.run([exe], input="".join(lines), capture_output=True, text=True, check=True).stdout.splitlines()


def test_the_key_file_compiled_for_the_host_gives_the_checkers_keys_digits_and_selection(tmp_path):
    run = _host_program(tmp_path)
    seeds = [0, 1, 1 << 32, 1 << 63, (1 << 63) + 12345, 12345, (1 << 64) - 1]
    cases = [(seed, s, r) for seed in seeds for s in (0, 1, 1147, (1 << 31) + 5, (1 << 32) - 1) for r in (0, 1, 255, 256, 65537, (1 << 31) - 2, (1 << 31) - 1)]
    assert len(cases) >= 200
    out = run("k %d %d %d 0\n" % c for c in cases)
    for c, line in zip(cases, out):
        v = [int(x) for x in line.split()]
        k = dc.key(*c)
        assert v[0] << 96 | v[1] << 64 | v[2] << 32 | v[3] == k, c
        assert v[4:] == [dc.digit(k, d) for d in range(16)], c                # all sixteen digits
    by = dict(zip(cases, out))
    assert by[(12345, 0, 0)] != by[((1 << 63) + 12345, 0, 0)] and by[(0, 0, 0)] != by[(1 << 32, 0, 0)]      # both key words are used
    assert by[(0, 0, 0)] != by[(0, 1, 0)] and by[(0, 0, 0)] != by[(0, 0, 1)] and len(set(out)) == len(out)
    # the selection on the file's helpers: ordinary inputs resolve within the first word, the searched ones go into the second
    picks = [(0, 0, 10, 3), (5, 3, 1000, 1), (5, 3, 1000, 999), (7, 1, 5000, 2500), (1 << 63, (1 << 32) - 1, 3000, 1234)] + SECOND_WORD[:2]
    for c, line in zip(picks, run("s %d %d %d %d\n" % c for c in picks)):
        v = [int(x) for x in line.split()]
        assert v[1:] == dc.kept_reads(*c).tolist(), c
        assert (v[0] >= 4) == (c in SECOND_WORD), (c, v[0])


def test_the_searched_cases_put_the_threshold_between_two_reads_that_share_the_first_word():
    for seed, s, M, n in SECOND_WORD:
        o0, o1, o2, o3 = dc.key_words(seed, s, np.arange(M))
        order = np.lexsort((o0, o1, o2, o3))
        assert o3[order[n - 1]] == o3[order[n]] and (o2[order[n - 1]], o1[order[n - 1]], o0[order[n - 1]]) != (o2[order[n]], o1[order[n]], o0[order[n]])
        assert 0 < n < M


# ---- 3. the moments of the rule ---------------------------------------------------------------------------------------------------------------
def test_the_kept_counts_have_the_hypergeometric_mean_and_variance():
    """Counts (1000, 3000, 6000), sample 3, n = 2000, seeds 0 .. 199.  Measured with these inputs: the means' z-scores 0.55, -1.09, 0.68; the
    largest single |z| 2.96; the lower half's z -0.34."""
    counts, s, n, B = np.array([1000, 3000, 6000]), 3, 2000, 200
    M = int(counts.sum())
    kept = np.array([dc.thin_column(counts, s, n, seed) for seed in range(B)])
    p = counts / M
    mean, var = n * p, n * p * (1 - p) * (M - n) / (M - 1)
    z = (kept.mean(axis=0) - mean) / np.sqrt(var / B)
    single = np.abs((kept - mean) / np.sqrt(var)).max()
    low = np.array([(dc.kept_reads(seed, s, M, n) < M // 2).sum() for seed in range(B)])
    z_low = (low.mean() - n / 2) / np.sqrt(n * 0.25 * (M - n) / (M - 1) / B)
    print("z of the means %s, largest single |z| %.2f, z of the lower half %.2f" % (np.round(z, 2), single, z_low))
    assert (kept.sum(axis=1) == n).all()
    assert (np.abs(z) < 4).all() and single < 5 and abs(z_low) < 4


# ---- 4. the header, the table, the build ------------------------------------------------------------------------------------------------------
def test_the_binding_has_tables_of_its_own_and_the_header_declares_its_symbols():
    hdr = open(os.path.join(ROOT, "include", "ecb_downsample.h")).read()
    main = open(os.path.join(ROOT, "include", "ecb.h")).read()
    assert sorted(set(re.findall(r"^int (ecb_\w+)\(", hdr, re.M))) == sorted(ed.DOWNSAMPLE_SYMBOLS) == ["ecb_downsample", "ecb_downsample_device"]
    assert [(s[0], len(s[1]), s[3]) for s in ed.DOWNSAMPLE_SIGNATURES] == [("ecb_downsample", 12, True)]
    for name, argtypes, _, _, _ in ed.DOWNSAMPLE_SIGNATURES:            # as many parameters as the prototypes have
        for n in (name, name + "_device"):
            assert len(re.search(r"^int %s\((.*?)\);" % n, hdr, re.M | re.S).group(1).split(",")) == len(argtypes), n
    assert not set(ed.DOWNSAMPLE_SYMBOLS) & set(ecb.SYMBOLS) and len(re.findall(r'^#\s*include "ecb_downsample\.h"', main, re.M)) == 1
    assert "ECB_ABI_VERSION 4" in main and "ecb_downsample" not in main.replace('"ecb_downsample.h"', "")
    assert "never share a key" in hdr and "no tie rule" in hdr                 # the kernels rely on it: the header says so
    from alntools_amd import build
    for f in ("ecb_downsample.h", "downsample.inc", "ds_key.h", "boot_draw.h"):
        assert any(p.endswith(f) for p in build.inputs()), f
    src = '#include "ecb.h"\nvoid* a = (void*)ecb_downsample; void* b = (void*)ecb_downsample_device;\n'
    r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = os.path.join(ROOT, "alntools_amd", "libecb.so")
    if os.path.exists(lib):                                      # the built library exports both
        import ctypes
        so = ctypes.CDLL(lib)
        for name in ed.DOWNSAMPLE_SYMBOLS:
            assert hasattr(so, name), name


def test_the_wrapper_reaches_its_symbol_once_behind_the_hook(monkeypatch):
    events = []

    class Lib(object):
        def __getattr__(self, name):
            if not name.startswith("ecb_"):
                raise AttributeError(name)
            return lambda *a: (events.append((name, len(a))), 0)[1]
    monkeypatch.setattr(ecb, "_lib", Lib())
    monkeypatch.setattr(ecb, "_tables", {})
    monkeypatch.setattr(ecb._Numpy, "ready", lambda self: events.append("ready"))
    out, tin, tout = ed.downsample([0, 2, 3], [0, 1, 1], [3, 4, 5], 2, [2, -1], seed=7)
    assert events == ["ready", ("ecb_downsample", 12)] and (len(out), len(tin), len(tout)) == (3, 2, 2)
    with pytest.raises(ValueError, match="target has 1 entries for 2 samples"):
        ed.downsample([0, 2, 3], [0, 1, 1], [3, 4, 5], 2, [2])
    with pytest.raises(ValueError, match="differ in length"):
        ed.downsample([0, 2, 3], [0, 1, 1], [3, 4], 2, [2, 1])


# ---- 5. the targets -------------------------------------------------------------------------------------------------------------------------
def test_the_targets_of_reads_fraction_and_equalize():
    totals, stay = np.array([10, 0, 7, 1000, 3, 2 ** 40 + 1]), np.array([True, False, True, True, False, True])
    assert bin_utils.downsample_targets(totals, stay, reads=8).tolist() == [8, -1, 8, 8, -1, 8]
    assert bin_utils.downsample_targets(totals, stay, equalize=True).tolist() == [7, -1, 7, 7, -1, 7]
    assert bin_utils.downsample_targets(totals, stay, fraction=0.5).tolist() == [5, -1, 3, 500, -1, 2 ** 39]
    assert bin_utils.downsample_targets(totals, stay, fraction=1.0).tolist() == [10, -1, 7, 1000, -1, 2 ** 40 + 1]
    assert bin_utils.downsample_targets(totals, stay, fraction=0.1).tolist() == [1, -1, 0, 100, -1, int(np.floor(np.float64(0.1) * np.float64(2 ** 40 + 1)))]
    assert bin_utils.downsample_targets([3, 29], [True, True], fraction=0.7).tolist() == [2, 20]          # floor of the float64 product: 0.7 x 3 = 2.0999...
    assert bin_utils.downsample_targets(totals, np.zeros(6, bool), equalize=True).tolist() == [-1] * 6
    for kw, text in ((dict(), "none is"), (dict(reads=3, fraction=0.5), "-n/--reads and -f/--fraction"), (dict(reads=3, equalize=True), "-n/--reads and --equalize"),
                     (dict(fraction=0.5, equalize=True), "-f/--fraction and --equalize"), (dict(reads=0), "at least 1"), (dict(reads=-4), "at least 1"),
                     (dict(fraction=0.0), "above 0 and at most 1"), (dict(fraction=1.5), "above 0 and at most 1"), (dict(fraction=float("nan")), "above 0")):
        with pytest.raises(ValueError, match=text):
            bin_utils.downsample_rule(**kw)
    assert [bin_utils.downsample_rule(reads=1), bin_utils.downsample_rule(fraction=1.0), bin_utils.downsample_rule(equalize=True)] == ["reads", "fraction", "equalize"]


def test_the_checkers_file_command_on_a_golden_file(golden_dir):
    m = bin_utils.ecload(os.path.join(golden_dir, "g4_multi_min0.bin"))
    M = dc.totals(m)
    n = int(np.sort(M)[len(M) // 2])
    out, stats = dc.ecdownsample(m, reads=n, seed=3)
    t = dc.totals(out)
    assert (M > 0).all() and out.sname == m.sname and t.tolist() == np.minimum(M, n).tolist() and (M > n).any() and (M <= n).any()
    assert [r[:3] for r in stats] == [(s, int(a), int(min(a, n))) for s, a in zip(m.sname, M)] and all(r[4] <= r[3] for r in stats)
    least = int(np.sort(M)[2])
    eq, _ = dc.ecdownsample(m, equalize=True, mincount=least)
    assert set(dc.totals(eq).tolist()) == {least} and eq.num_samples == int((M >= least).sum()) < m.num_samples
    assert np.array_equal(bin_utils.downsample_targets(M, dc.staying(m, None, 5), fraction=0.3), dc.targets(m, dc.staying(m, None, 5), fraction=0.3))


# ---- 6. bin_utils and the command line, the checkers in the device's place ------------------------------------------------------------------
def _fake_downsample(indptrN, indicesN, dataN, n_ecs, target, seed=0, device=0):
    return dc.downsample(indptrN, indicesN, dataN, n_ecs, target, seed)


def test_ecdownsample_with_the_checkers_as_the_device_writes_the_checkers_bytes(golden_dir, tmp_path, monkeypatch, caplog):
    monkeypatch.setattr(ecb, "select", _fake_select)
    monkeypatch.setattr(ed, "downsample", _fake_downsample)
    src, out, stats = os.path.join(golden_dir, "g4_multi_min0.bin"), str(tmp_path / "o.bin"), str(tmp_path / "s.tsv")
    m = bin_utils.ecload(src)
    with caplog.at_level("INFO", logger="alntools.utils"):
        bin_utils.ecdownsample(src, out, fraction=0.25, seed=11, samples=m.sname[1:6], mincount=2, stats_file=stats)
    exp, rows = dc.ecdownsample(m, fraction=0.25, seed=11, samples=m.sname[1:6], mincount=2)
    assert _bytes(out) == bin_utils.ecsave2_bytes(exp) and "samples: {:,} (from 8)".format(exp.num_samples) in caplog.text
    lines = open(stats).read().splitlines()
    assert lines[0].split("\t") == ["sample", "reads_in", "reads_out", "ecs_in", "ecs_out"]
    assert [tuple(ln.split("\t")) for ln in lines[1:]] == [tuple(str(v) for v in r) for r in rows] and len(rows) >= exp.num_samples > 0
    # a sample's result does not depend on which other samples were named
    bin_utils.ecdownsample(src, out, fraction=0.25, seed=11, samples=[m.sname[3]])
    one, both = bin_utils.ecload(out), exp
    k = both.sname.index(m.sname[3])
    assert one.sname == [m.sname[3]] and int(dc.totals(one)[0]) == int(dc.totals(both)[k])
    os.remove(out)
    os.remove(stats)
    for kw, text in ((dict(), "exactly one of"), (dict(reads=5, equalize=True), "exactly one of"), (dict(reads=0), "at least 1"),
                     (dict(fraction=2.0), "at most 1"), (dict(reads=5, samples=["nobody"]), "nobody"), (dict(reads=5, mincount=10 ** 9), "no sample left"),
                     (dict(fraction=1e-9), "no sample left")):
        with pytest.raises((ValueError, KeyError), match=text):
            bin_utils.ecdownsample(src, out, stats_file=stats, **kw)
        assert not os.path.exists(out) and not os.path.exists(stats)


def test_the_rule_is_refused_before_a_file_is_opened_or_the_library_loaded(tmp_path, monkeypatch):
    def never(*a, **k):
        raise AssertionError("reached")
    monkeypatch.setattr(bin_utils, "ecload", never)
    monkeypatch.setattr(ecb, "load", never)
    for kw in (dict(), dict(reads=1, fraction=0.5), dict(fraction=0.0), dict(reads=0)):
        with pytest.raises(ValueError):
            bin_utils.ecdownsample(str(tmp_path / "missing.bin"), str(tmp_path / "o.bin"), **kw)


def test_the_command_line_hands_its_options_to_methods(tmp_path, monkeypatch):
    from click.testing import CliRunner
    from alntools_amd import cli, methods
    e, names = tmp_path / "e.bin", tmp_path / "n.txt"
    e.write_bytes(b""); names.write_text("")
    o, st = str(tmp_path / "o.bin"), str(tmp_path / "s.tsv")
    seen = []
    monkeypatch.setattr(methods, "ecdownsample", lambda *a: seen.append(a))
    r = CliRunner().invoke(cli.cli, ["ecdownsample", str(e), o, "-n", "500", "--seed", "9", "-s", "a", "-s", "b", "--samples", str(names), "-m", "7",
                                     "--stats", st, "-v"])
    assert r.exit_code == 0, r.output
    assert CliRunner().invoke(cli.cli, ["ecdownsample", str(e), o, "--fraction", "0.5"]).exit_code == 0
    assert CliRunner().invoke(cli.cli, ["ecdownsample", str(e), o, "--equalize"]).exit_code == 0
    assert seen == [(str(e), o, 500, None, False, 9, ["a", "b"], str(names), 7, st), (str(e), o, None, 0.5, False, 0, None, None, None, None),
                    (str(e), o, None, None, True, 0, None, None, None, None)]

    def boom(*a):
        raise ValueError("no")
    monkeypatch.setattr(methods, "ecdownsample", boom)
    assert CliRunner().invoke(cli.cli, ["ecdownsample", str(e), o, "-n", "1"]).exit_code == 1


_RUN = """
import sys
sys.path[:0] = [%r, %r]
import test_ecdownsample as t
from alntools_amd import ecb, ecb_downsample, cli
ecb.select = t._fake_select
ecb_downsample.downsample = t._fake_downsample
cli.cli()
"""
REFUSALS = {"no_rule": ([], "exactly one of"), "reads_and_fraction": (["-n", "5", "-f", "0.5"], "exactly one of"),
            "reads_and_equalize": (["-n", "5", "--equalize"], "exactly one of"), "fraction_and_equalize": (["-f", "0.5", "--equalize"], "exactly one of"),
            "reads_0": (["-n", "0"], "at least 1"), "fraction_0": (["-f", "0"], "above 0"), "fraction_above_1": (["-f", "1.01"], "at most 1"),
            "unknown_sample": (["-n", "5", "-s", "CELL_NOPE"], "CELL_NOPE"), "unknown_sample_in_file": (["-n", "5", "--samples", "NAMES"], "CELL_NOPE"),
            "no_sample_left": (["-n", "5", "-m", "1000000"], "no sample left"), "thinned_to_nothing": (["-f", "0.000001"], "no sample left"),
            "not_a_bin": (["-n", "5"], None), "works": (["--equalize", "-m", "30", "--seed", "4", "--stats", "STATS"], None)}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_command_line_refusals_exit_1_and_write_nothing(golden_dir, tmp_path, what):
    out, stats, src = str(tmp_path / "out.bin"), str(tmp_path / "stats.tsv"), os.path.join(golden_dir, "g4_multi_min0.bin")
    names = tmp_path / "names.txt"
    m = bin_utils.ecload(src)
    names.write_text("%s\n\nCELL_NOPE\n" % m.sname[0])
    args, text = REFUSALS[what]
    args = [str(names) if a == "NAMES" else stats if a == "STATS" else a for a in args]
    if what == "not_a_bin":
        src = os.path.join(golden_dir, "g2_c1.range.txt")
    env = dict(os.environ)
    env.pop("ALNTOOLS_GPUS", None)
    r = subprocess.run([sys.executable, "-c", _RUN % (ROOT, os.path.join(ROOT, "tests")), "ecdownsample", src, out] + args + ["-v"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    if what == "works":
        assert r.returncode == 0, r.stderr
        exp, rows = dc.ecdownsample(m, equalize=True, mincount=30, seed=4)
        assert _bytes(out) == bin_utils.ecsave2_bytes(exp) and len(set(dc.totals(exp).tolist())) == 1
        assert open(stats).read().splitlines()[1:] == ["\t".join(str(v) for v in row) for row in rows]
        return
    assert r.returncode == 1, r.stdout + r.stderr
    assert not os.path.exists(out) and not os.path.exists(stats)
    assert "Error:" in r.stderr and "libecb" not in r.stderr, r.stderr
    assert text is None or text in r.stderr


def test_the_one_gpu_command_imports_no_pytorch():
    env = dict(os.environ)
    env.pop("ALNTOOLS_GPUS", None)
    env.pop("ALNTOOLS_TORCH", None)
    code = ("import sys; from alntools_amd import cli, bin_utils, methods; "
            "assert all(hasattr(x, 'ecdownsample') for x in (cli, bin_utils, methods)); print('torch' in sys.modules)")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "False", r.stdout + r.stderr
