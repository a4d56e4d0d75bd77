"""ecclusters without a GPU: the checker (``tests/components_checker.py``, scipy's ``connected_components``) against a pure-Python
union-find on random small cases and on every ``.bin`` under ``tests/golden/``, the component counts of the golden files as literals, the
ABI's header against the module's symbols, the text of the cluster file and of the stats table, what ``gene_ids`` and ``group_map`` make
of the file, and the command with the binding stood in by the checker: its files, and every refusal with no file left behind."""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from alntools_amd import bin_utils, ecb, ecb_components

import components_checker as cc
import counts_checker

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BINS = sorted(glob.glob(os.path.join(GOLDEN, "*.bin")))
_loaded = {}


@pytest.fixture(autouse=True)
def _logger_level_as_it_was():
    import logging
    log = logging.getLogger("alntools.utils")
    level = log.level
    yield
    log.setLevel(level)


def load(name):
    path = name if os.path.isabs(name) else os.path.join(GOLDEN, name)
    if path not in _loaded:
        _loaded[path] = bin_utils.ecload(path)
    return _loaded[path]


def args_of(m):
    return (m.indptrA, m.indicesA, m.dataA, m.num_loci, m.num_haplotypes, m.indptrN, m.indicesN, m.dataN)


# ---- 1. the checker against a union-find written out ---------------------------------------------------------------------------------------
def union_find(indptr, indices, data, n_loci, n_haps, indptr_n, indices_n, data_n, sample=None, min_count=1):
    """The definition of ``include/ecb_components.h`` in plain Python: the same six results as the checker, as lists and ints."""
    E, T = len(indptr) - 1, n_loci
    w = [0] * E
    lo, hi = (0, int(indptr_n[-1])) if sample is None else (int(indptr_n[sample]), int(indptr_n[sample + 1]))
    for j in range(lo, hi):
        w[int(indices_n[j])] += int(data_n[j])
    parent = list(range(T))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    members = [[int(indices[i]) for i in range(int(indptr[e]), int(indptr[e + 1])) if int(data[i]) != 0] for e in range(E)]
    links = [w[e] >= min_count and len(members[e]) > 0 for e in range(E)]
    for e in range(E):
        if links[e]:
            for t in members[e][1:]:
                a, b = find(members[e][0]), find(t)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    roots = sorted(set(find(t) for t in range(T)))                      # (the smaller root wins every union: a root is its component's smallest locus)
    number = {r: c for c, r in enumerate(roots)}
    of_locus = [number[find(t)] for t in range(T)]
    of_ec = [of_locus[members[e][0]] if links[e] else -1 for e in range(E)]
    C = len(roots)
    loci, ecs, reads = [0] * C, [0] * C, [0] * C
    for c in of_locus:
        loci[c] += 1
    for e in range(E):
        if links[e]:
            ecs[of_ec[e]] += 1
            reads[of_ec[e]] += w[e]
    return of_locus, of_ec, loci, ecs, reads, (C, sum(links), max(loci), sum(n >= 2 for n in loci))


def same(got, want, what=""):
    assert len(got) == len(want) == 6
    for name, g, e in zip(("comp_of_locus", "comp_of_ec", "comp_loci", "comp_ecs", "comp_reads"), got, want):
        assert list(np.asarray(g).tolist()) == list(np.asarray(e).tolist()), (what, name)
    assert tuple(got[5]) == tuple(want[5]), (what, "sizes")


def random_case(rng, E, T, H, S=1, zeros=0.0, absent=0.2):
    lens = np.minimum(rng.poisson(1.5, size=E), T)
    ip = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ix = np.concatenate([np.sort(rng.choice(T, size=int(n), replace=False)) for n in lens] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    da = rng.integers(1, 1 << H, size=len(ix)).astype(np.int32)
    da[rng.random(len(ix)) < zeros] = 0
    cols = [np.flatnonzero(rng.random(E) >= absent) for _ in range(S)]
    pn = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    xn = np.concatenate(cols + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    dn = rng.integers(0, 6, size=len(xn)).astype(np.int32)
    return ip, ix, da, T, H, pn, xn, dn


@pytest.mark.parametrize("seed", range(12))
def test_the_checker_is_a_union_find_on_random_small_cases(seed):
    rng = np.random.default_rng(seed)
    E, T, S = int(rng.integers(0, 60)), int(rng.integers(1, 50)), int(rng.integers(1, 4))
    a = random_case(rng, E, T, 3, S=S, zeros=0.3 if seed % 2 else 0.0)
    for sample in [None] + list(range(S)):
        for mc in (0, 1, 3):
            got = cc.components(*a, sample=sample, min_count=mc)
            same(got, union_find(*a, sample=sample, min_count=mc), (seed, sample, mc))
            assert got[0][0] == 0 and (got[0] <= np.arange(T)).all() and got[0].dtype == np.int32 and got[4].dtype == np.int64


@pytest.mark.parametrize("path", BINS, ids=[os.path.basename(p) for p in BINS])
def test_the_checker_is_a_union_find_on_every_golden_bin(path):
    m = load(path)
    for mc in (1, 2):
        same(cc.components(*args_of(m), min_count=mc), union_find(*args_of(m), min_count=mc), mc)
    if m.num_samples > 1:
        same(cc.components(*args_of(m), sample=m.num_samples - 1), union_find(*args_of(m), sample=m.num_samples - 1))


# ---- 2. the golden files' components -------------------------------------------------------------------------------------------------------
def test_the_components_of_the_golden_files():
    m = load("g2_c1.bin")
    assert cc.components(*args_of(m), min_count=1)[5] == (40, 3313, 416, 25)
    assert cc.components(*args_of(m), min_count=2)[5] == (580, 1278, 131, 65)
    s = cc.components(*args_of(m), min_count=5)[5]
    assert (s[0], s[3], s[2]) == (930, 14, 36)
    s = cc.components(*args_of(load("gt_h8.out.bin")))[5]
    assert (s[0], s[3], s[2]) == (1175, 1, 2826)
    ms = load("gt_ms.out.bin")
    assert [cc.components(*args_of(ms), sample=c)[5][0] for c in (None, 0, 5)] == [15, 19, 28]
    long = cc.components(*args_of(load("salmon_long.bin")))
    assert long[5][0] == 1 and long[5][2] == 1500 and not long[0].any()


def test_the_checkers_weights_are_count_alignments():
    m = load("gt_ms.out.bin")
    w = counts_checker.weights(m.num_reads, m.indptrN, m.indicesN, m.dataN)
    got = cc.components(*args_of(m))
    assert int(got[4].sum()) == int(w[got[1] >= 0].sum()) and got[5][1] == int((got[1] >= 0).sum())


# ---- 3. the header and the bindings ----------------------------------------------------------------------------------------------------------
def test_the_header_declares_exactly_the_modules_symbols():
    text = open(os.path.join(ROOT, "include", "ecb_components.h")).read()
    declared = re.findall(r"^int (ecb_\w+)\(", text, re.M)
    assert sorted(declared) == sorted(ecb_components.COMPONENTS_SYMBOLS) and len(set(declared)) == 2
    main = open(os.path.join(ROOT, "include", "ecb.h")).read()
    assert len(re.findall(r'^#\s*include "ecb_components\.h"', main, re.M)) == 1 and "ECB_ABI_VERSION 4" in main and ecb.ABI_VERSION == 4
    assert "ecb_components" not in main.replace('"ecb_components.h"', "") and "ABI 4, additive" in text
    bound = [n for name, _, _, twin, _ in ecb_components.COMPONENTS_SIGNATURES for n in ((name + "_device", name) if twin else (name,))]
    assert sorted(bound) == sorted(ecb_components.COMPONENTS_SYMBOLS)
    assert not set(ecb_components.COMPONENTS_SYMBOLS) & set(ecb.SYMBOLS)
    assert not {s[0] for s in ecb.SIGNATURES} & {s[0] for s in ecb_components.COMPONENTS_SIGNATURES}
    for name, argtypes, _, _, _ in ecb_components.COMPONENTS_SIGNATURES:          # as many parameters as the prototypes have
        for n in (name, name + "_device"):
            proto = re.search(r"^int %s\((.*?)\);" % n, text, re.M | re.S).group(1)
            assert len(proto.split(",")) == len(argtypes) == 21, n
    from alntools_amd import build
    assert any(p.endswith("ecb_components.h") for p in build.inputs()) and any(p.endswith("components.inc") for p in build.inputs())
    # a C compiler sees them through ecb.h alone
    src = '#include "ecb.h"\nvoid* a = (void*)ecb_components; void* b = (void*)ecb_components_device;\n'
    r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_library_exports_both_entry_points_and_refuses_before_a_device_is_touched():
    import ctypes as C
    lib = ecb_components.load()
    lib.ecb_last_error.restype = C.c_char_p
    buf = (C.c_int64 * 16)()
    p = C.cast(buf, C.c_void_p)
    sizes = (C.c_uint64 * 4)(7, 7, 7, 7)
    ARG, LIMIT, CONTRACT = -1, -8, -5
    for fn in (lib.ecb_components, lib.ecb_components_device):
        def call(min_count=1, sample=-1, of_locus=p, out=sizes, nnz=4, n_haps=2):
            return fn(0, 2, 3, n_haps, nnz, p, p, p, 1, 2, p, p, p, sample, min_count, of_locus, p, p, p, p, out)
        assert call(min_count=-1) == ARG and b"min_count" in lib.ecb_last_error(None)
        assert call(of_locus=None) == ARG and call(out=None) == ARG and call(n_haps=32) == ARG
        assert call(nnz=1 << 30) == LIMIT
        assert call(sample=1) == CONTRACT and call(sample=-2) == CONTRACT
        assert list(sizes) == [7, 7, 7, 7]


# ---- 4. the files ------------------------------------------------------------------------------------------------------------------------------
def test_the_text_of_the_cluster_file_and_of_the_stats_table():
    names = ["t0", "t1", "t2", "t3", "t4", "t5"]
    comp = np.array([0, 1, 0, 2, 1, 0], dtype=np.int32)
    text, written = bin_utils.clusters_file(names, comp)
    assert text == "t0\tt0\tt2\tt5\nt1\tt1\tt4\nt3\tt3\n" and list(written) == [0, 1, 2]
    text, written = bin_utils.clusters_file(names, comp, multi_only=True)
    assert text == "t0\tt0\tt2\tt5\nt1\tt1\tt4\n" and list(written) == [0, 1]
    stats = bin_utils.clusters_stats(written, [3, 2, 1], [4, 1, 0], [1 << 40, 5, 0])
    assert stats == "cluster\ttargets\tecs\treads\n0\t3\t4\t%d\n1\t2\t1\t5\n" % (1 << 40)
    assert bin_utils.clusters_stats([2], [3, 2, 1], [4, 1, 0], [9, 5, 0]) == "cluster\ttargets\tecs\treads\n2\t1\t0\t0\n"
    # two targets of one name: refused when both would head a line, and only then
    dup = ["a", "b", "a", "c"]
    with pytest.raises(ValueError, match="named a "):
        bin_utils.clusters_file(dup, np.array([0, 1, 2, 1]))
    assert bin_utils.clusters_file(dup, np.array([0, 1, 2, 1]), multi_only=True)[0] == "b\tb\tc\n"
    assert bin_utils.clusters_file(dup, np.array([0, 1, 0, 1]))[0] == "a\ta\ta\nb\tb\tc\n"


def _stand_in(monkeypatch, calls):
    def components(*a, **kw):
        calls.append(kw)
        kw = dict(kw)
        kw.pop("device")
        return cc.components(*a, **kw)
    monkeypatch.setattr(ecb_components, "components", components)


def partition(labels):
    """A labelling as the set of its classes."""
    groups = {}
    for t, g in enumerate(labels):
        groups.setdefault(int(g), []).append(t)
    return sorted(groups.values())


@pytest.mark.parametrize("name,argv,kw", [
    ("g2_c1.bin", [], {}), ("g2_c1.bin", ["-m", "2"], {"min_count": 2}), ("gt_ms.out.bin", ["-s", "sample5"], {"sample": 5}),
    ("gt_h8.out.bin", ["-m", "0"], {"min_count": 0}), ("salmon_long.bin", [], {}),
], ids=["c1", "c1-m2", "ms-s5", "h8-m0", "long"])
def test_the_command_with_the_binding_stood_in_writes_what_gene_ids_and_group_map_read_back(tmp_path, monkeypatch, name, argv, kw):
    from click.testing import CliRunner
    from alntools_amd import cli
    calls = []
    _stand_in(monkeypatch, calls)
    m = load(name)
    if "-s" in argv:
        argv = ["-s", m.sname[kw["sample"]]]
    want = cc.components(*args_of(m), **kw)
    out, multi, stats = (str(tmp_path / f) for f in ("all.grp.txt", "multi.grp.txt", "stats.tsv"))
    r = CliRunner().invoke(cli.cli, ["ecclusters", os.path.join(GOLDEN, name), out, "--stats", stats] + argv)
    assert r.exit_code == 0, r.output
    assert calls[0]["min_count"] == kw.get("min_count", 1) and calls[0]["sample"] == kw.get("sample") and calls[0]["device"] == 0
    lines = open(out).read().split("\n")
    C = want[5][0]
    assert lines[-1] == "" and len(lines) == C + 1
    first = [int(np.flatnonzero(want[0] == c)[0]) for c in range(C)]
    for c in (0, C // 2, C - 1):
        assert lines[c].split("\t") == [m.lname[first[c]]] + [m.lname[t] for t in np.flatnonzero(want[0] == c)]
    # the default file: gene_ids numbers the targets as comp_of_locus does, group_map takes it and loses no target
    gene, names = bin_utils.gene_ids(m, out)
    assert np.array_equal(gene, want[0]) and names == [m.lname[t] for t in first]
    gname, map_ptr, map_idx, _ = bin_utils.group_map(m, out)
    assert gname == names and np.array_equal(np.diff(map_ptr), np.ones(m.num_loci)) and np.array_equal(map_idx, want[0])
    table = [ln.split("\t") for ln in open(stats).read().split("\n")]
    assert table[0] == ["cluster", "targets", "ecs", "reads"] and table[-1] == [""] and len(table) == C + 2
    assert [[int(v) for v in row] for row in table[1:-1]] == [[c, int(want[2][c]), int(want[3][c]), int(want[4][c])] for c in range(C)]
    # --multi-only: the same partition to gene_ids, the singletons off the file and off the table
    r = CliRunner().invoke(cli.cli, ["ecclusters", os.path.join(GOLDEN, name), multi, "--multi-only", "--stats", stats] + argv)
    assert r.exit_code == 0, r.output
    kept = [c for c in range(C) if want[2][c] >= 2]
    assert len(open(multi).read().split("\n")) == len(kept) + 1 == want[5][3] + 1
    assert partition(bin_utils.gene_ids(m, multi)[0]) == partition(want[0])
    assert [int(ln.split("\t")[0]) for ln in open(stats).read().split("\n")[1:-1]] == kept
    assert "``ecclusters``" in cli.__doc__ and "alntools ecclusters sample.bin clusters.grp.txt" in open(os.path.join(ROOT, "README.md")).read()
    from alntools_amd import methods
    assert "``ecclusters``" in methods.__doc__


def test_verbose_logs_the_sizes(tmp_path, monkeypatch, caplog):
    import logging
    _stand_in(monkeypatch, [])
    with caplog.at_level(logging.INFO, logger="alntools.utils"):
        bin_utils.ecclusters(os.path.join(GOLDEN, "g2_c1.bin"), str(tmp_path / "c.grp.txt"))
    text = "\n".join(r.getMessage() for r in caplog.records)
    assert "Number of clusters: 40 (25 of two targets or more), from 3,313 linking ECs" in text
    assert "Largest cluster: 416 targets (41.6% of the targets)" in text


@pytest.mark.parametrize("argv,text,code", [
    (["-m", "-1"], "must be at least 0", 1), (["-s", "nobody"], "sample nobody is not in", 1), (["-m", "x"], None, 2),
], ids=["negative-m", "unknown-sample", "m-not-a-number"])
def test_a_refusal_comes_before_the_library_and_leaves_no_file(tmp_path, monkeypatch, argv, text, code, caplog):
    from click.testing import CliRunner
    from alntools_amd import cli

    def never(*a, **kw):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(ecb_components, "components", never)
    monkeypatch.setattr(ecb, "load", never)
    out, stats = str(tmp_path / "c.grp.txt"), str(tmp_path / "stats.tsv")
    r = CliRunner().invoke(cli.cli, ["ecclusters", os.path.join(GOLDEN, "gt_ms.out.bin"), out, "--stats", stats] + argv)
    assert r.exit_code == code, r.output
    assert os.listdir(str(tmp_path)) == []
    if text:
        assert any(text in rec.getMessage() and rec.getMessage().startswith("Error: ") for rec in caplog.records)
    with pytest.raises(ValueError):
        bin_utils.ecclusters(os.path.join(GOLDEN, "g2_c1.bin"), out, min_count=-1)
    with pytest.raises(KeyError):
        bin_utils.ecclusters(os.path.join(GOLDEN, "g2_c1.bin"), out, sample="nobody")
    assert os.listdir(str(tmp_path)) == []


def test_two_heads_of_one_name_are_refused_and_a_failure_behind_the_first_file_removes_it(tmp_path, monkeypatch):
    _stand_in(monkeypatch, [])
    m = load("g1_edge.bin")
    of_locus = cc.components(*args_of(m))[0]
    heads = [int(np.flatnonzero(of_locus == c)[0]) for c in range(int(of_locus.max()) + 1)]
    assert len(heads) >= 2
    twin = bin_utils.ECMatrices(m.hname, [m.lname[heads[0]] if t == heads[1] else n for t, n in enumerate(m.lname)], m.lengths, m.sname,
                                m.indptrA, m.indicesA, m.dataA, m.indptrN, m.indicesN, m.dataN)
    src = str(tmp_path / "twin.bin")
    bin_utils.ecsave2(src, twin)
    out, stats = str(tmp_path / "c.grp.txt"), str(tmp_path / "stats.tsv")
    with pytest.raises(ValueError, match="named %s " % re.escape(m.lname[heads[0]])):
        bin_utils.ecclusters(src, out, stats_file=stats)
    assert sorted(os.listdir(str(tmp_path))) == ["twin.bin"]
    with pytest.raises(OSError):
        bin_utils.ecclusters(os.path.join(GOLDEN, "g1_edge.bin"), str(tmp_path / "no-such-dir" / "c.grp.txt"), stats_file=stats)
    assert sorted(os.listdir(str(tmp_path))) == ["twin.bin"]
