"""ecbundle on the GPU (``ecb_bundle`` / ``ecb_bundle_device``) against the bundle checker, byte for byte: the recorded golden cases
through ``bin_utils.ecbundle``, seeded random inputs and groupings, runs of equal (row, group) keys on the wave and workgroup boundaries
of the fold kernel, pair counts on the scan tile, rows around the table's inline-pair limit, the collapse of rows and counts, every
contract violation refused with its outputs untouched, and ``ecb.combine`` unchanged by the steps it now shares."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from alntools_amd import bin_utils, ecb

import bundle_checker as bchk
import ec_merge_checker as chk
from test_bundle_constants import FOLD_TPB, INL, SCAN_TILE, WAVE

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "bundle_cases.json")))["cases"]
RECORDED = [c for c in CASES if c["raises"] is None]


def _bytes(p):
    with open(p, "rb") as f:
        return f.read()


def _names(n, p="g"):
    return ["%s%d" % (p, i) for i in range(n)]


def _device(m, gname, groups):
    """ecb.bundle over an ECMatrices and per-group member lists -> the bytes ecbundle would write."""
    ptr, idx = bchk.group_csr(m.num_loci, groups)
    out = ecb.bundle(m.indptrA, m.indicesA, m.dataA, m.indptrN, m.indicesN, m.dataN, m.num_loci, m.num_haplotypes, len(gname), ptr, idx)
    return bin_utils.ecsave2_bytes(bin_utils.ECMatrices(m.hname, gname, bchk.group_lengths(m, groups), m.sname, *out))


def _agree(m, gname, groups):
    assert _device(m, gname, groups) == bchk.bundle_bytes(m, gname, groups)


def _m(rows, H, T, counts=None, sname=("s",)):
    """ECMatrices from rows of (columns, masks); counts[s][e] (default: every row once in every sample)."""
    ip = np.cumsum([0] + [len(r[0]) for r in rows])
    ix = np.concatenate([np.asarray(r[0], dtype=np.int64) for r in rows] + [np.zeros(0, np.int64)])
    dx = np.concatenate([np.asarray(r[1], dtype=np.int64) for r in rows] + [np.zeros(0, np.int64)])
    counts = [[1] * len(rows) for _ in sname] if counts is None else counts
    ipn, ixn, dxn = [0], [], []
    for c in counts:
        nz = [e for e, v in enumerate(c) if v]
        ixn += nz
        dxn += [c[e] for e in nz]
        ipn.append(len(ixn))
    lens = np.arange(T * H).reshape(T, H) % 977 + 50
    return bin_utils.ECMatrices(_names(H, "h"), _names(T, "t"), lens, list(sname), ip, ix, dx, ipn, ixn, dxn)


# ---- 1. goldens -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in RECORDED if c["name"] != "c1"], ids=lambda c: c["name"])
def test_golden_cases_through_ecbundle(golden_dir, tmp_path, case):
    ec, grp, out = os.path.join(golden_dir, case["ec"]), os.path.join(golden_dir, case["grp"]), str(tmp_path / "o.bin")
    bin_utils.ecbundle(ec, grp, out)
    m = bin_utils.ecload(ec)
    assert _bytes(out) == bchk.bundle_bytes(m, *bin_utils.load_groups(m, grp))
    assert bin_utils.ecload(out).num_reads < m.num_reads


def test_golden_c1_whose_group_file_repeats_a_name_is_refused_by_the_command_and_bundled_by_the_library(golden_dir, tmp_path):
    ec, out = os.path.join(golden_dir, "g2_c1.bin"), str(tmp_path / "o.bin")
    with pytest.raises(ValueError, match="G00003"):
        bin_utils.ecbundle(ec, os.path.join(golden_dir, "gt_c1.grp.txt"), out)
    with pytest.raises(KeyError):
        bin_utils.ecbundle(ec, os.path.join(golden_dir, "gt_err_tx.grp.txt"), out)
    assert not os.path.exists(out)
    m = bin_utils.ecload(ec)
    _agree(m, *bin_utils.load_groups(m, os.path.join(golden_dir, "gt_c1.grp.txt")))       # (the map itself is well formed)


def test_the_command_line_bundles_without_pytorch(golden_dir, tmp_path):
    case = next(c for c in CASES if c["name"] == "c1_mixed")
    ec, grp, out = os.path.join(golden_dir, case["ec"]), os.path.join(golden_dir, case["grp"]), str(tmp_path / "o.bin")
    env = dict(os.environ)
    env.pop("ALNTOOLS_GPUS", None)
    env["ALNTOOLS_TORCH"] = "0"
    r = subprocess.run([sys.executable, "-m", "alntools_amd.cli", "ecbundle", ec, grp, out, "-v"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    m = bin_utils.ecload(ec)
    exp = bchk.bundle(m, *bin_utils.load_groups(m, grp))
    assert _bytes(out) == bin_utils.ecsave2_bytes(exp)
    assert "Number of equivalence classes: {:,} (from {:,} rows)".format(exp.num_reads, m.num_reads) in r.stderr


# ---- 2. random --------------------------------------------------------------------------------------------------------------------------
def _grouping(kind, rng, T):
    if kind == "own":
        return [[t] for t in range(T)]
    if kind == "one":
        return [list(range(T))]
    if kind == "g1":                                                        # G = 1, a third of the loci in no group
        return [[t for t in range(T) if rng.random() < 0.67]]
    G = T // 3 + 7                                                          # loci in 0, 1 and 3 groups; groups without a member
    groups = [[] for _ in range(G)]
    for t in range(T):
        k = (0, 1, 1, 3)[int(rng.integers(0, 4))]
        for g in rng.choice(G - 5, size=k, replace=False):                  # (the last five groups stay empty)
            groups[int(g)].append(t)
    return groups


@pytest.mark.parametrize("kind", ["mixed", "g1", "own", "one"])
@pytest.mark.parametrize("H,sname", [(1, ["s"]), (2, ["s", "u", "v"]), (8, ["s"]), (31, ["s", "u"])])
def test_random_inputs_and_groupings(H, sname, kind):
    rng = np.random.default_rng(1000 * H + len(kind) + len(sname))
    T = 300
    m = chk.random_bin(rng, 1500, _names(T, "t"), _names(H, "h"), sname, max_row=250)
    groups = _grouping(kind, rng, T)
    _agree(m, _names(len(groups)), groups)


def test_device_tensors_go_through_the_device_entry():
    import torch
    rng = np.random.default_rng(5)
    T, H = 200, 4
    m = chk.random_bin(rng, 800, _names(T, "t"), _names(H, "h"), ["s", "u"], max_row=150)
    groups = _grouping("mixed", rng, T)
    ptr, idx = bchk.group_csr(T, groups)
    dev = [torch.as_tensor(np.asarray(a, dtype=np.int32), device="cuda") for a in (m.indptrA, m.indicesA, m.dataA, m.indptrN, m.indicesN, m.dataN, ptr, idx)]
    out = ecb.bundle(*dev[:6], T, H, len(groups), dev[6], dev[7])
    assert all(o.is_cuda for o in out)
    got = bin_utils.ECMatrices(m.hname, _names(len(groups)), bchk.group_lengths(m, groups), m.sname, *[o.cpu().numpy() for o in out])
    assert bin_utils.ecsave2_bytes(got) == bchk.bundle_bytes(m, _names(len(groups)), groups)


# ---- 3. the fold --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, WAVE - 1, WAVE, WAVE + 1, 2 * WAVE + 2, FOLD_TPB + 44])
def test_runs_on_the_wave_and_workgroup_boundaries_of_the_fold(L):
    """Sorted pairs: per placement a filler row of single pairs (runs of 1), then a row whose L loci are all in one group -- one run of L
    that starts at the wanted offset within the fold's workgroup.  Starts and ends on, one before and one after a wave boundary (64) and
    a workgroup boundary (256); the last run is the last thing in the array."""
    F = FOLD_TPB                                                           # loci 0 .. F-1: groups of their own; F .. F+L-1: all in group F
    T, H = F + L, 8
    groups = [[t] for t in range(F)] + [list(range(F, F + L))]
    starts = set()
    for B in (WAVE, FOLD_TPB):
        for d in (-1, 0, 1):
            starts.add((B + d) % FOLD_TPB)                                 # the run starts around the boundary
            starts.add((B - L + d) % FOLD_TPB)                             # ... ends around it
    rng = np.random.default_rng(L)
    rows, pos = [], 0
    for s in sorted(starts):
        n = (s - pos) % FOLD_TPB
        rows.append((np.arange(n), rng.integers(1, 1 << H, n)))
        masks = 1 << rng.integers(0, H, L)                                 # single bits: the OR shows which members arrived
        rows.append((np.arange(F, F + L), masks))
        pos += n + L
    m = _m(rows, H, T)
    u = bchk.uncollapsed(m, _names(F + 1), groups)
    assert u.indicesA[-1] == F and len(u.indicesA) == sum(len(r[0]) for r in rows[0::2]) + len(starts)
    run_starts = np.cumsum([0] + [len(r[0]) for r in rows])[1::2] % FOLD_TPB
    assert sorted(run_starts.tolist()) == sorted(starts)
    _agree(m, _names(F + 1), groups)


# ---- 4. scan and expansion boundaries -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_locus", [1, 2])
@pytest.mark.parametrize("X", [SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1])
def test_pair_counts_on_the_scan_tile(X, per_locus):
    """X expanded pairs; with one group per locus the non-zeros sit on the tile of the scan in front of the expansion too."""
    rng = np.random.default_rng(X + per_locus)
    T, H = 64, 2
    groups = [[t] for t in range(T)] + ([[1]] + [[t, t + 1] for t in range(2, T, 2)] if per_locus == 2 else [])      # (locus 0: one group)
    ptr, _ = bchk.group_csr(T, groups)
    rows, x = [], 0
    while x < X:
        keep = []
        for c in np.sort(rng.choice(T, size=8, replace=False)):
            k = int(ptr[c + 1] - ptr[c])
            if x + k <= X:
                keep.append(c)
                x += k
        rows.append((np.array(keep, dtype=np.int64), rng.integers(1, 1 << H, len(keep))))
    m = _m(rows, H, T)
    assert int((ptr[1:] - ptr[:-1])[m.indicesA].sum()) == X and (per_locus == 2 or len(m.indicesA) == X)
    _agree(m, _names(len(groups)), groups)


def test_nothing_to_bundle():
    H, T = 2, 10
    groups = [[0, 1], [2]]
    _agree(_m([], H, T, counts=[[]]), _names(2), groups)                                                    # E = 0
    _agree(_m([((), ())] * 5, H, T, counts=[[1, 0, 2, 0, 3]]), _names(2), groups)                          # nnz = 0
    rows = [((3, 4), (1, 2)), ((5,), (3,)), ((), ())]
    _agree(_m(rows, H, T, counts=[[1, 2, 0], [0, 4, 5]], sname=("s", "u")), _names(2), groups)            # every row bundles to empty
    _agree(_m(rows, H, T), _names(3), [[], [], []])                                                         # a map without an entry


def test_rows_around_the_inline_pair_limit():
    H, T = 4, 40
    groups = [[t for t in range(T) if t % 3 == g] for g in range(3)] + [[t] for t in range(20, 40)]
    rows = [(np.arange(0, INL + 3), np.arange(1, INL + 4) % 15 + 1),        # above INL before, 3 pairs after
            (np.arange(0, 2 * INL), [1] * (2 * INL)),                        # the same groups, other masks
            (np.arange(18, 18 + INL + 4), [2] * (INL + 4)),                  # above INL after the fold: 3 + 7 groups
            (np.arange(20, 20 + INL - 3), [4] * (INL - 3)),                  # 2 loci in 4 groups: below INL
            (np.arange(20, 22), [4, 4])]
    m = _m(rows, H, T, counts=[[1, 2, 3, 4, 5]])
    b = bchk.bundle(m, _names(len(groups)), groups)
    lens = np.diff(b.indptrA).tolist()
    assert lens[0] == 3 and lens[1] == 3 and max(lens) > INL and min(lens) <= INL
    _agree(m, _names(len(groups)), groups)


# ---- 5. collapse and N --------------------------------------------------------------------------------------------------------------------
def test_rows_that_agree_after_the_bundle_share_an_ec_and_add_their_counts():
    H, T = 2, 8
    groups = [[0, 1, 2], [3, 4], [5]]                                       # (6 and 7 in no group)
    rows = [((0,), (1,)), ((1,), (1,)), ((0, 2), (1, 1)), ((3,), (2,)), ((4, 6), (2, 3)), ((6, 7), (1, 1)), ((), ()), ((2, 5), (1, 3))]
    counts = [[1, 2, 4, 0, 8, 16, 0, 32], [0, 0, 5, 0, 0, 7, 9, 0], [3, 0, 0, 0, 0, 0, 0, 0]]          # rows 3 is counted by no sample
    m = _m(rows, H, T, counts=counts, sname=("s", "u", "v"))
    b = bchk.bundle(m, _names(3), groups)
    assert b.num_reads == 4 and b.indptrA.tolist() == [0, 1, 2, 2, 4]
    assert b.indptrN.tolist() == [0, 4, 6, 7] and b.dataN.tolist() == [7, 8, 16, 32, 5, 16, 3]
    assert int(b.dataN.sum()) == int(m.dataN.sum())                         # counts >= 0: no sum is 0, the checker drops nothing
    _agree(m, _names(3), groups)


def test_a_summed_count_of_int32_max_passes_and_one_more_is_refused():
    H, T = 2, 4
    rows = [((0,), (1,)), ((1,), (1,)), ((2,), (2,))]
    top = 2 ** 31 - 1
    m = _m(rows, H, T, counts=[[top - 5, 5, 1]])
    _agree(m, _names(2), [[0, 1], [2]])
    out = ecb.bundle(m.indptrA, m.indicesA, m.dataA, m.indptrN, m.indicesN, m.dataN, T, H, 2, *bchk.group_csr(T, [[0, 1], [2]]))
    assert out[5].tolist() == [top, 1]
    m = _m(rows, H, T, counts=[[top - 5, 6, 1]])
    with pytest.raises(ecb.EcbError) as e:
        _device(m, _names(2), [[0, 1], [2]])
    assert e.value.code == -8 and "a merged count exceeds int32" in str(e.value)


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------
FILL = 0x5A5A5A5A


def _raw(a, n_loci, n_haps, n_groups, cap):
    """ecb_bundle itself on pre-filled outputs: (return code, message, the outputs)."""
    lib = ecb.load()
    a = {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in a.items()}
    E, S = len(a["indptrA"]) - 1, len(a["indptrN"]) - 1
    outs = [np.full(n, FILL, dtype=np.int32) for n in (E + 1, cap, cap, S + 1, max(len(a["indicesN"]), 1), max(len(a["indicesN"]), 1))]
    sizes = (C.c_uint64 * 3)(7, 7, 7)
    p = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    rc = lib.ecb_bundle(0, E, n_loci, n_haps, S, n_groups, len(a["indicesA"]), p(a["indptrA"]), p(a["indicesA"]), p(a["dataA"]), len(a["indicesN"]),
                        p(a["indptrN"]), p(a["indicesN"]), p(a["dataN"]), len(a["map_idx"]), p(a["map_ptr"]), p(a["map_idx"]), cap,
                        *([p(o) for o in outs] + [sizes]))
    return rc, (lib.ecb_last_error(None) or b"").decode(), outs


def test_contract_violations_are_refused_with_the_outputs_untouched_and_the_next_call_works():
    rng = np.random.default_rng(11)
    T, H, G = 300, 3, 80
    m = chk.random_bin(rng, 500, _names(T, "t"), _names(H, "h"), ["s", "u"], max_row=200, long_share=0.05, empty_share=0.0)
    groups = [[] for _ in range(G)]
    for t in range(T):
        for g in rng.choice(G, size=int(rng.integers(0, 4)), replace=False):
            groups[int(g)].append(t)
    ptr, idx = bchk.group_csr(T, groups)
    good = dict(indptrA=m.indptrA, indicesA=m.indicesA, dataA=m.dataA, indptrN=m.indptrN, indicesN=m.indicesN, dataN=m.dataN, map_ptr=ptr, map_idx=idx)
    cap = int((ptr[1:] - ptr[:-1])[m.indicesA].sum())
    exp = bchk.bundle(m, _names(G), groups)
    long_row = int(np.argmax(np.diff(m.indptrA)))
    s0 = int(m.indptrA[long_row])
    wide = int(np.argmax(np.diff(ptr) >= 2))                                # a locus in two groups or more
    w0 = int(ptr[wide])
    A_PTR = "malformed CSR A: row pointers do not start at 0, go backwards or do not end at nnz"
    A_ORDER = "malformed CSR A: columns not strictly ascending within a row"
    M_PTR = "malformed group map: pointers do not start at 0, go backwards or do not end at the number of group ids"
    M_ORDER = "malformed group map: group ids not strictly ascending within a locus (unsorted or duplicate)"
    bad = []

    def case(what, code, text, **kw):
        for k, (at, v) in list(kw.items()):
            x = np.array(good[k]).copy()
            x[at] = v
            kw[k] = x
        bad.append((what, dict(good, **kw), code, text))
    case("a map pointer that falls", -5, M_PTR, map_ptr=(slice(10, 12), [ptr[11] + 1, ptr[10]] if ptr[11] > ptr[10] else [ptr[10] + 1, ptr[10]]))
    case("map_ptr[0] != 0", -5, M_PTR, map_ptr=(0, 1))
    case("map_ptr[T] != len(map_idx)", -5, M_PTR, map_ptr=(-1, ptr[-1] - 1))
    case("map_ptr[T] beyond len(map_idx)", -5, M_PTR, map_ptr=(-1, ptr[-1] + 1))
    case("a negative map pointer", -5, M_PTR, map_ptr=(5, -3))
    case("a group id at n_groups", -5, "malformed group map: a group id at or beyond n_groups", map_idx=(w0, G))
    case("unsorted groups within a locus", -5, M_ORDER, map_idx=(slice(w0, w0 + 2), [idx[w0 + 1], idx[w0]]))
    case("a duplicate group within a locus", -5, M_ORDER, map_idx=(w0 + 1, idx[w0]))
    case("column >= T", -5, "malformed CSR A: a column at or beyond the part's n_loci", indicesA=(5, T))
    case("negative column", -5, "malformed CSR A: a column at or beyond the part's n_loci", indicesA=(7, -1))
    case("bit >= H", -5, "malformed CSR A: a stored 0 or a haplotype bit at or beyond n_haplotypes", dataA=(9, 8))
    case("stored 0", -5, "malformed CSR A: a stored 0 or a haplotype bit at or beyond n_haplotypes", dataA=(11, 0))
    case("unsorted column", -5, A_ORDER, indicesA=(slice(s0 + 1, s0 + 3), [m.indicesA[s0 + 2], m.indicesA[s0 + 1]]))
    case("duplicate column", -5, A_ORDER, indicesA=(s0 + 2, m.indicesA[s0 + 1]))
    case("falling indptr", -5, A_PTR, indptrA=(slice(10, 12), [m.indptrA[11], m.indptrA[10]]))
    case("indptr[E] != nnz", -5, A_PTR, indptrA=(-1, m.indptrA[-1] - 1))
    case("indptr[0] != 0", -5, A_PTR, indptrA=(0, 1))
    case("EC index >= E", -5, "malformed CSC N: an EC index at or beyond the part's n_ecs", indicesN=(3, m.num_reads))
    case("negative count", -5, "malformed CSC N: a negative count", dataN=(4, -2))
    case("N pointers", -5, "malformed CSC N: column pointers do not start at 0, go backwards or do not end at nnz", indptrN=(-1, m.indptrN[-1] + 1))
    assert m.indptrA[10] != m.indptrA[11]
    for what, a, code, text in bad:
        rc, msg, outs = _raw(a, T, H, G, cap)
        assert rc == code and text in msg, (what, rc, msg)
        assert all(np.all(o == FILL) for o in outs), what
    rc, msg, outs = _raw(good, T, H, G, len(exp.indicesA) - 1)             # too little room for A: refused before anything is written
    assert rc == -1 and "room for" in msg and all(np.all(o == FILL) for o in outs)
    rc, msg, outs = _raw(good, T, H, G, cap)                                # the device is unharmed
    assert rc == 0, msg
    n_out = len(exp.indptrA)                                                # the folded ECs' pointers: fewer than the E + 1 there is room for
    assert n_out < len(outs[0]) and np.array_equal(outs[0][:n_out], exp.indptrA) and np.all(outs[0][n_out:] == FILL)
    assert np.array_equal(outs[1][:len(exp.indicesA)], exp.indicesA)
    assert np.array_equal(outs[2][:len(exp.dataA)], exp.dataA) and np.array_equal(outs[3], exp.indptrN)
    assert np.all(outs[1][len(exp.indicesA):] == FILL) and np.all(outs[2][len(exp.dataA):] == FILL)
    _agree(m, _names(G), groups)


def test_a_locus_in_more_groups_than_the_scan_can_count_is_refused():
    G = 65536
    m = _m([((0,), (1,))], 1, 1)
    with pytest.raises(ecb.EcbError) as e:
        ecb.bundle(m.indptrA, m.indicesA, m.dataA, m.indptrN, m.indicesN, m.dataN, 1, 1, G, [0, G], np.arange(G))
    assert e.value.code == -8 and "a locus in more than 65535 groups" in str(e.value)
    out = ecb.bundle(m.indptrA, m.indicesA, m.dataA, m.indptrN, m.indicesN, m.dataN, 1, 1, G, [0, G - 1], np.arange(G - 1))
    assert out[0].tolist() == [0, G - 1] and np.array_equal(out[1], np.arange(G - 1)) and np.all(out[2] == 1)


# ---- 7. ecb.combine, which now shares its steps -----------------------------------------------------------------------------------------
def test_combine_gives_the_bytes_it_gave(golden_dir):
    def combine(ms):
        plan = bin_utils.plan_merge(ms)
        parts = [dict(indptrA=x.indptrA, indicesA=x.indicesA, dataA=x.dataA, indptrN=x.indptrN, indicesN=x.indicesN, dataN=x.dataN,
                      n_loci=x.num_loci, target_map=tm, sample_map=sm) for x, tm, sm in zip(ms, plan.target_maps, plan.sample_maps)]
        return bin_utils.ecsave2_bytes(bin_utils.ECMatrices(plan.hname, plan.lname, plan.lengths, plan.sname,
                                                            *ecb.combine(parts, len(plan.lname), len(plan.hname), len(plan.sname))))
    p = os.path.join(golden_dir, "g2_c1.bin")
    assert combine([bin_utils.ecload(p)]) == _bytes(p)
    rng = np.random.default_rng(21)
    a = chk.random_bin(rng, 900, _names(400, "t"), ["A", "B", "C"], ["s1", "s2"], max_row=300)
    b = chk.permute_targets(chk.random_bin(rng, 700, _names(400, "t"), ["A", "B", "C"], ["s2", "s3"], max_row=300), rng)
    b.lengths = np.asarray(a.lengths)[[a.lname.index(t) for t in b.lname]]
    c = chk.random_bin(rng, 300, _names(400, "t"), ["A", "B", "C"], ["s4"], max_row=30)
    c.lengths = a.lengths
    assert combine([a, b, c]) == chk.merge_bytes([a, b, c])
