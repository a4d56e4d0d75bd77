"""ecselect on the GPU (``ecb_select`` / ``ecb_select_device``) against the select checker, byte for byte: the reference's thresholded
``.bin`` files through the command, the recorded files under every class, seeded random matrices through both entry points, every size on
the edges of the scan's stretch, rows and columns across the work boundaries of the passes, every contract violation refused with its
outputs untouched, all of it once more with the scratch poisoned, and ``ecb_count_alignments`` on what ``--unique`` wrote."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from alntools_amd import bin_utils, ecb

import ec_merge_checker as chk
import select_checker as schk
from test_select_constants import SCAN_TILE, SHARE

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = json.load(open(os.path.join(GOLDEN, "select_cases.json")))["cases"]
THRESHOLDED = [("g4_multi_min0.bin", 20, "g4_multi_min20.bin"), ("g4_multi_min0.bin", 60, "g4_multi_min60.bin"),
               ("g4b_multi_min0.bin", 40, "g4b_multi_min40.bin"), ("g4b_multi_min0.bin", 160, "g4b_multi_min160.bin"),
               ("g4_multi_min20.bin", 60, "g4_multi_min60.bin"), ("g4_multi_min0.bin", 0, "g4_multi_min0.bin")]
EDGES = [SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 1]


def _bytes(p):
    with open(p, "rb") as f:
        return f.read()


def _names(n, p):
    return ["%s%d" % (p, i) for i in range(n)]


def _mat(H, T, indptrA, indicesA, dataA, indptrN, indicesN, dataN):
    S = len(indptrN) - 1
    return bin_utils.ECMatrices(_names(H, "h"), _names(T, "t"), np.zeros((T, H)), _names(S, "s"), indptrA, indicesA, dataA, indptrN, indicesN, dataN)


def _device(m, row_class=None, keep=None, mincount=None, tensors=False):
    """ecb.select over an ECMatrices -> (the ECMatrices ecselect would write, the samples that stayed)."""
    a = [m.indptrA, m.indicesA, m.dataA, m.indptrN, m.indicesN, m.dataN]
    if tensors:
        import torch
        a = [torch.as_tensor(np.asarray(x, dtype=np.int32), device="cuda") for x in a]
    out, stay = ecb.select(*a, m.num_loci, m.num_haplotypes, row_class=row_class, sample_keep=keep, min_count=mincount)
    if tensors:
        assert all(o.is_cuda for o in out) and stay.is_cuda
        out, stay = [o.cpu().numpy() for o in out], stay.cpu().numpy()
    return bin_utils.ECMatrices(m.hname, m.lname, m.lengths, [s for s, k in zip(m.sname, stay) if k], *out), np.asarray(stay, dtype=bool)


def _agree(m, row_class=None, keep=None, mincount=None, tensors=False):
    exp, stay, rows = schk.select_flags(m, row_class, keep, mincount)
    got, gstay = _device(m, row_class, keep, mincount, tensors)
    assert np.array_equal(gstay, stay)
    for k in ("indptrA", "indicesA", "dataA", "indptrN", "indicesN", "dataN"):
        assert np.array_equal(getattr(got, k), getattr(exp, k)), k
    assert bin_utils.ecsave2_bytes(got) == bin_utils.ecsave2_bytes(exp)
    return exp, stay, rows


# ---- 1. goldens ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,m,dst", THRESHOLDED, ids=["%s-m%d" % (t[0][:-4], t[1]) for t in THRESHOLDED])
def test_a_threshold_gives_the_references_thresholded_file(tmp_path, src, m, dst):
    out = str(tmp_path / "o.bin")
    bin_utils.ecselect(os.path.join(GOLDEN, src), out, mincount=m)
    assert _bytes(out) == _bytes(os.path.join(GOLDEN, dst))


def _some_dropped(m, row_class):
    """A threshold that drops some samples and keeps some: above the smallest total; one sample: above its total (none is left)."""
    total = np.zeros(m.num_samples, dtype=np.int64)
    cls = schk.in_class(m, row_class)
    col = np.repeat(np.arange(m.num_samples), np.diff(m.indptrN))
    np.add.at(total, col[cls[m.indicesN]], m.dataN[cls[m.indicesN]].astype(np.int64))
    return int(np.sort(total)[len(total) // 2]) + 1


@pytest.mark.parametrize("row_class", schk.CLASSES, ids=lambda c: c or "all")
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_recorded_files_under_every_class_with_and_without_a_threshold(tmp_path, case, row_class):
    src, out = os.path.join(GOLDEN, case["ec"]), str(tmp_path / "o.bin")
    m = bin_utils.ecload(src)
    for mincount in (None, _some_dropped(m, row_class)):
        exp, stay, rows = _agree(m, row_class, None, mincount)
        if mincount is None and row_class in ("unique", "locus-unique"):
            assert int(rows.sum()) == case["rows"]["allele" if row_class == "unique" else "locus"]
        if mincount is not None:
            assert not stay.all() and (stay.any() or m.num_samples == 1)
        if exp.num_samples and exp.num_reads:
            bin_utils.ecselect(src, out, row_class=row_class, mincount=mincount)
            assert _bytes(out) == bin_utils.ecsave2_bytes(exp)
            os.remove(out)
        else:
            with pytest.raises(ValueError, match="no sample left" if not exp.num_samples else "no read left"):
                bin_utils.ecselect(src, out, row_class=row_class, mincount=mincount)
            assert not os.path.exists(out)


def test_the_command_line_selects_without_pytorch(tmp_path):
    src, out, names = os.path.join(GOLDEN, "g4b_multi_min0.bin"), str(tmp_path / "o.bin"), tmp_path / "n.txt"
    m = bin_utils.ecload(src)
    picked = m.sname[5:300:2]
    names.write_text("\n".join(picked[3:]) + "\n\n")
    env = dict(os.environ)
    env.pop("ALNTOOLS_GPUS", None)
    env["ALNTOOLS_TORCH"] = "0"
    cmd = [sys.executable, "-m", "alntools_amd.cli", "ecselect", src, out, "--locus-unique", "-s", picked[2], "-s", picked[0], "-s", picked[1],
           "--samples", str(names), "-m", "5", "-v"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    exp = schk.select(m, "locus-unique", picked, 5)
    assert _bytes(out) == bin_utils.ecsave2_bytes(exp) and 0 < exp.num_samples < len(picked)
    assert "ECs: {:,} (from {:,} rows)".format(exp.num_reads, m.num_reads) in r.stderr
    assert "samples: {:,} (from {:,})".format(exp.num_samples, m.num_samples) in r.stderr
    r = subprocess.run(cmd[:6] + ["-s", "CELL_NOPE"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "CELL_NOPE" in r.stderr


# ---- 2. random ----------------------------------------------------------------------------------------------------------------------------
def _random(seed, H, S, E=1500, T=300):
    """A seeded matrix with stored 0 masks, rows nobody counts, zero counts, ECs listed twice in a column and empty columns."""
    rng = np.random.default_rng(seed)
    a = chk.random_bin(rng, E, _names(T, "t"), _names(H, "h"), ["x"], max_row=250, long_share=0.03)
    d = np.array(a.dataA, dtype=np.int64)
    d[rng.random(len(d)) < 0.15] = 0
    single = rng.random(len(d)) < 0.5                                       # one bit only: allele-unique rows are not rare
    d[single] &= -d[single]
    if H == 31 and len(d):
        d[int(rng.integers(0, len(d)))] = 1 << 30
    ip, ix, dx = [0], [], []
    for s in range(S):
        n = 0 if rng.random() < 0.1 else int(rng.integers(1, max(2, (2 * E) // max(1, min(S, 40)))))
        ec = np.sort(rng.integers(0, E, n))                                 # (with repeats)
        c = rng.integers(0, 60, n)
        c[rng.random(n) < 0.15] = 0
        ix.append(ec); dx.append(c); ip.append(ip[-1] + n)
    m = _mat(H, T, a.indptrA, a.indicesA, d, ip, np.concatenate(ix), np.concatenate(dx))
    keep = None if seed % 3 == 0 else rng.random(S) < 0.7
    return m, keep, rng


RANDOM = [(H, S) for H in (1, 2, 8, 31) for S in (1, 3, 338)]


def _random_case(H, S, tensors=False):
    m, keep, rng = _random(100 * H + S, H, S)
    for row_class in schk.CLASSES:
        _agree(m, row_class, keep, None, tensors)
        total = np.sort(np.bincount(np.repeat(np.arange(S), np.diff(m.indptrN)), weights=m.dataN, minlength=S))
        _agree(m, row_class, keep, int(total[S // 2] * 0.4) + int(rng.integers(0, 3)), tensors)
    if H == 31:
        assert (m.dataA == 1 << 30).any()


@pytest.mark.parametrize("H,S", RANDOM)
def test_random_matrices_through_the_host_entry(H, S):
    _random_case(H, S)


@pytest.mark.parametrize("H,S", [(2, 3), (31, 338)])
def test_random_matrices_as_device_tensors_go_through_the_device_entry(H, S):
    _random_case(H, S, tensors=True)


# ---- 3. sizes on the scan's stretch -------------------------------------------------------------------------------------------------------
def _rows_of_len(lens, T, H, rng):
    """CSR A with the given row lengths: columns start .. start + len - 1 (ascending), masks random and not 0."""
    lens = np.asarray(lens, dtype=np.int64)
    ip = np.concatenate([[0], np.cumsum(lens)])
    start = rng.integers(0, T - lens + 1)
    ix = np.arange(ip[-1]) - np.repeat(ip[:-1], lens) + np.repeat(start, lens)
    return ip, ix, rng.integers(1, 1 << H, ip[-1])


def _pattern(kind, E):
    k = np.zeros(E, dtype=bool)
    if kind == "all":
        k[:] = True
    elif kind == "first":
        k[0] = True
    elif kind == "last":
        k[-1] = True
    elif kind == "alternating":
        k[::2] = True
    return k


def _edge_case(what, n):
    rng = np.random.default_rng(n + len(what))
    H, T = 2, 50
    if what in ("all", "none", "first", "last", "alternating"):            # E = n rows, those of the pattern counted by the one sample
        lens = np.ones(n, dtype=np.int64); lens[0] = 3
        counted = np.flatnonzero(_pattern(what, n))
        m = _mat(H, T, *_rows_of_len(lens, T, H, rng), [0, len(counted)], counted, rng.integers(1, 9, len(counted)))
        exp, stay, rows = _agree(m)
        assert m.num_reads == n and exp.num_reads == len(counted)
    elif what == "nnzA":                                                    # n non-zeros in rows of 1 .. 9, all kept
        lens = []
        while sum(lens) < n:
            lens.append(min(int(rng.integers(1, 10)), n - sum(lens)))
        E = len(lens)
        m = _mat(H, T, *_rows_of_len(lens, T, H, rng), [0, E], np.arange(E), np.ones(E))
        exp = _agree(m)[0]
        assert len(m.indicesA) == n == len(exp.indicesA)
    elif what == "nnzN":                                                    # n entries of N in three samples, the middle one dropped
        E = n // 2
        ec = np.concatenate([np.sort(rng.integers(0, E, k)) for k in (n // 3, n // 3, n - 2 * (n // 3))])
        m = _mat(H, T, *_rows_of_len(np.ones(E), T, H, rng), [0, n // 3, 2 * (n // 3), n], ec, rng.integers(1, 9, n))
        exp = _agree(m, None, [True, False, True])[0]
        assert len(m.indicesN) == n and 0 < len(exp.indicesN) < n
    elif what == "kept_rows":                                               # exactly n of 2 n + 5 rows stay
        E = 2 * n + 5
        counted = np.sort(rng.choice(E, n, replace=False))
        m = _mat(H, T, *_rows_of_len(rng.integers(0, 3, E), T, H, rng), [0, n], counted, np.ones(n))
        exp = _agree(m)[0]
        assert exp.num_reads == n
    elif what == "kept_N":                                                  # exactly n of 2 n + 3 entries stay
        E, nn = 500, 2 * n + 3
        c = np.zeros(nn, dtype=np.int64); c[rng.choice(nn, n, replace=False)] = rng.integers(1, 9, n)
        cut = int(rng.integers(1, nn))
        ec = np.concatenate([np.sort(rng.integers(0, E, cut)), np.sort(rng.integers(0, E, nn - cut))])
        m = _mat(H, T, *_rows_of_len(np.ones(E), T, H, rng), [0, cut, nn], ec, c)
        exp = _agree(m)[0]
        assert len(exp.indicesN) == n
    elif what == "S+1":                                                     # n column pointers: n - 1 samples of 0 .. 2 entries, a third named
        S, E = n - 1, 700
        per = rng.integers(0, 3, S)
        ip = np.concatenate([[0], np.cumsum(per)])
        ec = np.concatenate([np.sort(rng.choice(E, k, replace=False)) for k in per] + [np.zeros(0, np.int64)])
        m = _mat(H, T, *_rows_of_len(np.ones(E), T, H, rng), ip, ec, rng.integers(1, 5, ip[-1]))
        exp, stay, rows = _agree(m, None, rng.random(S) < 0.34, 2)
        assert len(m.indptrN) == n and 0 < stay.sum() < S
    else:
        raise KeyError(what)


EDGE_WHAT = ["all", "none", "first", "last", "alternating", "nnzA", "nnzN", "kept_rows", "kept_N", "S+1"]


@pytest.mark.parametrize("n", EDGES)
@pytest.mark.parametrize("what", EDGE_WHAT)
def test_sizes_on_the_scans_stretch(what, n):
    _edge_case(what, n)


def test_nothing_to_select():
    rng = np.random.default_rng(3)
    _agree(_mat(2, 5, [0], [], [], [0, 0], [], []))                                                          # E = 0
    _agree(_mat(2, 5, [0, 0, 0, 0], [], [], [0, 2, 2], [0, 2], [1, 4]), None, None, 3)                     # nnz(A) = 0: empty rows are rows
    _agree(_mat(2, 5, *_rows_of_len([2, 1, 3], 5, 2, rng), [0, 0, 0], [], []), "multi")                    # nnz(N) = 0
    _agree(_mat(2, 5, *_rows_of_len([2, 1, 3], 5, 2, rng), [0, 2, 3], [0, 2, 1], [1, 4, 2]), None, [False, False])      # no sample named


# ---- 4. rows and columns across the work boundaries ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first", "last", "dropped_between_two_kept"])
@pytest.mark.parametrize("L", [SHARE + SHARE // 2, SCAN_TILE + 700])
def test_rows_across_the_work_boundaries(L, where):
    """One row longer than a workgroup's share of the gather (1024 non-zeros), or than the scan's stretch; runs of empty rows at both ends."""
    rng = np.random.default_rng(L)
    H, T = 4, L + 50
    small = [int(x) for x in rng.integers(1, 7, 40)]
    lens = {"first": [L] + small, "last": small + [L], "dropped_between_two_kept": small[:20] + [5, L, 3] + small[20:]}[where]
    lens = [0] * 9 + lens + [0] * 11
    E = len(lens)
    big = lens.index(L)
    counted = np.ones(E, dtype=bool)
    counted[rng.random(E) < 0.3] = False
    counted[big] = where != "dropped_between_two_kept"
    if where == "dropped_between_two_kept":
        counted[big - 1] = counted[big + 1] = True
    counted[[0, 1, E - 1]] = [True, False, True]                           # an empty row may stay: class "all" keeps what is counted
    rows = np.flatnonzero(counted)
    m = _mat(H, T, *_rows_of_len(lens, T, H, rng), [0, len(rows)], rows, rng.integers(1, 9, len(rows)))
    exp, stay, kept = _agree(m)
    assert bool(kept[big]) == (where != "dropped_between_two_kept") and kept[0] and kept[E - 1] and not kept[1]
    _agree(m, "multi")
    _agree(m, "locus-unique")


def test_columns_across_the_work_boundaries():
    rng = np.random.default_rng(17)
    H, T, E = 2, 40, 3000
    A = _rows_of_len(rng.integers(0, 4, E), T, H, rng)
    # empty columns first, last and side by side; one column with all of N, several workgroups long
    n = 3 * SHARE + 77
    ec = np.sort(rng.integers(0, E, n))
    m = _mat(H, T, *A, [0, 0, 0, n, n, n], ec, rng.integers(0, 9, n))
    for row_class in schk.CLASSES:
        _agree(m, row_class)
        _agree(m, row_class, None, 1)
        _agree(m, row_class, [True, False, True, True, False])
    # columns that end inside a thread's four entries and inside a workgroup's share
    cuts = np.array([0, 1, 2, 3, 5, 6, SHARE - 1, SHARE, SHARE + 1, SHARE + 2, 2 * SHARE + 3, n])
    m = _mat(H, T, *A, cuts, np.concatenate([np.sort(ec[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]), rng.integers(0, 9, n))
    _agree(m, None, None, 4)
    _agree(m, "multi", rng.random(len(cuts) - 1) < 0.6, 3)


def test_a_total_above_2_to_the_32_is_summed_in_64_bits():
    rng = np.random.default_rng(23)
    H, T, E = 2, 10, 2 * SHARE + 9
    top = 2 ** 31 - 1
    A = _rows_of_len(np.ones(E), T, H, rng)
    c0 = np.full(E, top, dtype=np.int64)                                    # one column several workgroups long: its total is split
    c1 = np.array([top, top, 3], dtype=np.int64)
    m = _mat(H, T, *A, [0, E, E + 3], np.concatenate([np.arange(E), [4, 9, E - 1]]), np.concatenate([c0, c1]))
    t0, t1 = E * top, 2 * top + 3
    assert t1 > 2 ** 32 and t0 > 2 ** 32
    for mincount, names in ((t1 - 1, ["s0", "s1"]), (t1, ["s0", "s1"]), (t1 + 1, ["s0"]), (t0, ["s0"]), (t0 + 1, [])):
        exp = _agree(m, None, None, mincount)[0]
        assert exp.sname == names, mincount
    assert _agree(m, None, None, (t1 + 1) % 2 ** 32)[0].sname == ["s0", "s1"]        # (what a 32-bit total would have made of it)


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------
FILL = 0x5A5A5A5A


def _raw(a, n_loci, n_haps, row_class=0, keep=None, mincount=-1, null=()):
    """ecb_select itself on pre-filled outputs: (return code, message, the outputs)."""
    lib = ecb.load()
    a = {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in a.items()}
    E, S, nnz, nnz_n = len(a["indptrA"]) - 1, len(a["indptrN"]) - 1, len(a["indicesA"]), len(a["indicesN"])
    outs = [np.full(n, FILL, dtype=np.int32) for n in (E + 1, nnz, nnz, S + 1, nnz_n, nnz_n)] + [np.full(S, 0x5A, dtype=np.uint8)]
    sizes = (C.c_uint64 * 4)(7, 7, 7, 7)
    p = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    ptrs = [None if k in null else p(o) for k, o in enumerate(outs)]
    rc = lib.ecb_select(0, E, n_loci, n_haps, S, nnz, p(a["indptrA"]), p(a["indicesA"]), p(a["dataA"]), nnz_n, p(a["indptrN"]), p(a["indicesN"]),
                        p(a["dataN"]), row_class, None if keep is None else p(keep), mincount, *(ptrs + [None if 7 in null else sizes]))
    return rc, (lib.ecb_last_error(None) or b"").decode(), outs, list(sizes)


def _untouched(outs, sizes):
    return all(np.all(o == FILL) for o in outs[:6]) and np.all(outs[6] == 0x5A) and sizes == [7, 7, 7, 7]


def test_contract_violations_are_refused_with_the_outputs_untouched_and_the_next_call_works():
    m, _, rng = _random(7, 3, 4, E=600, T=200)
    T, H = m.num_loci, m.num_haplotypes
    good = dict(indptrA=m.indptrA, indicesA=m.indicesA, dataA=m.dataA, indptrN=m.indptrN, indicesN=m.indicesN, dataN=m.dataN)
    nnz, nnz_n, E, S = len(m.indicesA), len(m.indicesN), m.num_reads, m.num_samples
    lens = np.diff(m.indptrA)
    two = np.flatnonzero(lens >= 2)                                         # rows in which two columns can be swapped or repeated
    assert len(two) >= 3
    A_PTR = "malformed CSR: row pointers do not start at 0, go backwards or do not end at nnz"
    A_ORDER = "malformed CSR: columns not strictly ascending within a row"
    N_PTR = "malformed N: column pointers do not start at 0, go backwards or do not end at nnz_n"
    bad = []

    def case(what, text, **kw):
        for k, (at, v) in list(kw.items()):
            x = np.array(good[k]).copy()
            x[at] = v
            kw[k] = x
        bad.append((what, dict(good, **kw), text))
    mid_e = int(np.flatnonzero(lens > 0)[len(np.flatnonzero(lens > 0)) // 2])
    for name, at in (("first", 0), ("middle", nnz // 2), ("last", nnz - 1)):
        case("column >= T, " + name, "malformed CSR: a locus at or beyond n_loci", indicesA=(at, T))
        case("negative column, " + name, "malformed CSR: a locus at or beyond n_loci", indicesA=(at, -1))
        case("bit >= H, " + name, "malformed CSR: a haplotype bit at or beyond n_haplotypes", dataA=(at, 1 << H))
    for name, r in (("first", two[0]), ("middle", two[len(two) // 2]), ("last", two[-1])):
        s0 = int(m.indptrA[r])
        case("unsorted columns, %s row with two" % name, A_ORDER, indicesA=(slice(s0, s0 + 2), [m.indicesA[s0 + 1], m.indicesA[s0]]))
        case("duplicate column, %s row with two" % name, A_ORDER, indicesA=(s0 + 1, m.indicesA[s0]))
    case("indptr[0] != 0", A_PTR, indptrA=(0, 1))
    case("a falling row pointer in the middle", A_PTR, indptrA=(slice(mid_e, mid_e + 2), [m.indptrA[mid_e + 1], m.indptrA[mid_e]]))
    case("a negative row pointer", A_PTR, indptrA=(mid_e, -4))
    case("indptr[E] below nnz", A_PTR, indptrA=(-1, nnz - 1))
    case("indptr[E] beyond nnz", A_PTR, indptrA=(-1, nnz + 1))
    for name, at in (("first", 0), ("middle", nnz_n // 2), ("last", nnz_n - 1)):
        case("EC index at E, " + name, "malformed N: an EC index at or beyond n_ecs", indicesN=(at, E))
        case("negative EC index, " + name, "malformed N: an EC index at or beyond n_ecs", indicesN=(at, -1))
        case("negative count, " + name, "malformed N: a negative count", dataN=(at, -2))
    case("N's first pointer", N_PTR, indptrN=(0, 1))
    case("N's pointers fall in the middle", N_PTR, indptrN=(slice(1, 3), [m.indptrN[2] + 1, m.indptrN[1]] if m.indptrN[2] == m.indptrN[1]
                                                           else [m.indptrN[2], m.indptrN[1]]))
    case("N's last pointer below nnz_n", N_PTR, indptrN=(-1, nnz_n - 1))
    case("N's last pointer beyond nnz_n", N_PTR, indptrN=(-1, nnz_n + 1))
    keep = np.array([1, 0, 1, 1], dtype=np.uint8)
    for what, a, text in bad:
        for row_class, k, mc in ((0, None, -1), (1, keep, 5)):
            rc, msg, outs, sizes = _raw(a, T, H, row_class, k, mc)
            assert rc == -5 and text in msg, (what, rc, msg)
            assert _untouched(outs, sizes), what
    for what, kw in (("row_class 4", dict(row_class=4)), ("row_class -1", dict(row_class=-1)), ("no out_indptr_a", dict(null=(0,))),
                     ("no out_indices_a", dict(null=(1,))), ("no out_data_n", dict(null=(5,))), ("no out_sample_keep", dict(null=(6,))),
                     ("no out_sizes", dict(null=(7,)))):
        rc, msg, outs, sizes = _raw(good, T, H, **kw)
        assert rc == -1 and _untouched(outs, sizes), (what, rc, msg)
    rc, msg, outs, sizes = _raw(good, T, H, 3, keep, 5)                     # the call after a refusal: the device is unharmed
    assert rc == 0, msg
    exp, stay, rows = schk.select_flags(m, "multi", keep != 0, 5)
    assert sizes == [exp.num_reads, len(exp.indicesA), exp.num_samples, len(exp.indicesN)] and np.array_equal(outs[6] != 0, stay)
    for o, e in zip(outs, (exp.indptrA, exp.indicesA, exp.dataA, exp.indptrN, exp.indicesN, exp.dataN)):
        assert np.array_equal(o[:len(e)], e) and np.all(o[len(e):] == FILL)      # only the result's part of every output is written
    assert 0 < exp.num_reads < E and 0 < exp.num_samples < S


# ---- 6. the scratch poisoned --------------------------------------------------------------------------------------------------------------
def _all_random_and_edge_cases():
    for H, S in RANDOM:
        _random_case(H, S)
    for what in EDGE_WHAT:
        for n in EDGES:
            _edge_case(what, n)
    test_nothing_to_select()
    test_columns_across_the_work_boundaries()
    print("poisoned cases done")


def test_the_random_and_edge_cases_with_the_scratch_poisoned():
    """One child process with ECB_POISON_SCRATCH=1: every buffer the library allocates is filled with 0x01 first, so a pass that relied on
    fresh memory being 0 gives another answer than the checker's."""
    env = dict(os.environ)
    env["ECB_POISON_SCRATCH"] = "1"
    env["ALNTOOLS_TORCH"] = "0"
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_ecselect as t; t._all_random_and_edge_cases()" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "poisoned cases done" in r.stdout


# ---- 7. count-alignments on what --unique wrote -------------------------------------------------------------------------------------------
def test_count_alignments_of_the_unique_reads_is_the_unique_count_of_the_input(tmp_path):
    src, out = os.path.join(GOLDEN, "g4b_multi_min0.bin"), str(tmp_path / "u.bin")
    m = bin_utils.ecload(src)
    args = lambda x: (x.indptrA, x.indicesA, x.dataA, x.num_loci, x.num_haplotypes, x.indptrN, x.indicesN, x.dataN)   # noqa: E731
    _, uniq_in, lu_in = ecb.count_alignments(*args(m))
    bin_utils.ecselect(src, out, row_class="unique")
    aln, uniq, _ = ecb.count_alignments(*args(bin_utils.ecload(out)))
    assert np.array_equal(aln, uniq) and np.array_equal(uniq, uniq_in) and uniq_in.sum() > 0
    bin_utils.ecselect(src, out, row_class="locus-unique")
    assert np.array_equal(ecb.count_alignments(*args(bin_utils.ecload(out)))[2], lu_in) and lu_in.sum() > 0
