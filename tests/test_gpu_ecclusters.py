"""ecclusters on the GPU (``ecb_components`` / ``ecb_components_device``): every output compared exactly with the checker
(``tests/components_checker.py``: scipy's ``connected_components``, held to a union-find in ``test_ecclusters.py``).  The golden files through
the binding on numpy arrays and on CUDA tensors, ``bin_utils.ecclusters`` and the command line; the shapes at which a concurrent union-find
goes wrong; row lengths around the hook pass's items per thread and per workgroup (``test_components_constants.py``); masks of 0; weights;
degenerate inputs; one rule for every route; every break of A's and N's contract; and ``ecbundle`` on the cluster file.

All shapes stay at or below T = 20 000 loci and 200 000 non-zeros."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from alntools_amd import bin_utils, ecb, ecb_components

import components_checker as cc
import gt_checker
from test_components_constants import CC_ITEMS, CC_WG_ITEMS
from test_ecclusters import GOLDEN, args_of, load

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ARG, CONTRACT = -1, -5
NAMES = ("comp_of_locus", "comp_of_ec", "comp_loci", "comp_ecs", "comp_reads")
DTYPES = (np.int32, np.int32, np.int32, np.int32, np.int64)
_kept = {}


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _run(a, tensors=False, **kw):
    """``ecb_components.components`` on numpy arrays or on CUDA tensors -> numpy arrays and the sizes."""
    ip, ix, da, T, H, pn, xn, dn = a
    if tensors:
        import torch
        ip, ix, da, pn, xn, dn = (torch.as_tensor(np.ascontiguousarray(v, dtype=np.int32), device="cuda") for v in (ip, ix, da, pn, xn, dn))
    out = ecb_components.components(ip, ix, da, T, H, pn, xn, dn, **kw)
    if tensors:
        assert all(t.is_cuda for t in out[:5])
    return tuple(_np(t) for t in out[:5]) + (out[5],)


def _same(got, want, what=""):
    for name, dt, g, e in zip(NAMES, DTYPES, got, want):
        assert g.dtype == dt and g.shape == np.asarray(e).shape, (what, name, g.dtype, g.shape)
        assert np.array_equal(g, e), (what, name, int((g != e).sum()))
    assert tuple(got[5]) == tuple(want[5]), (what, got[5], want[5])


def _check(a, what="", **kw):
    """Both entry points against the checker; -> the checker's result."""
    want = cc.components(*a, **kw)
    _same(_run(a, **kw), want, (what, "host"))
    _same(_run(a, tensors=True, **kw), want, (what, "device"))
    return want


def _ones(E):
    """N of one sample in which every EC counts one read."""
    return np.array([0, E], dtype=np.int32), np.arange(E, dtype=np.int32), np.ones(E, dtype=np.int32)


def _csr(rows, T, H=2, masks=None, N=None):
    """Rows (each a list of ascending loci) -> the eight arguments; every mask 1 unless ``masks`` gives them per row."""
    lens = [len(r) for r in rows]
    ip = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ix = np.array([t for r in rows for t in r], dtype=np.int32)
    da = np.ones(len(ix), dtype=np.int32) if masks is None else np.array([v for r in masks for v in r], dtype=np.int32)
    assert len(da) == len(ix) and all(list(r) == sorted(set(r)) for r in rows) and (not len(ix) or ix.max() < T)
    return (ip, ix, da, T, H) + tuple(_ones(len(rows)) if N is None else N)


def _pairs(a, b, T, order=None):
    """Rows {a[k], b[k]} (a[k] != b[k]), in the order given."""
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    k = np.arange(len(lo)) if order is None else order
    ix = np.stack([lo[k], hi[k]], axis=1).reshape(-1).astype(np.int32)
    E = len(lo)
    return (np.arange(0, 2 * E + 1, 2, dtype=np.int32), ix, np.ones(2 * E, dtype=np.int32), T, 2) + _ones(E)


# ---- the golden files, through three routes --------------------------------------------------------------------------------------------------
#: (file, sample column, min_count)
GOLDENS = [("g2_c1.bin", None, 1), ("g2_c1.bin", None, 2), ("g2_c1.bin", None, 5), ("gt_h8.out.bin", None, 1), ("gt_ms.out.bin", None, 1),
           ("gt_ms.out.bin", 0, 1), ("gt_ms.out.bin", 5, 1), ("salmon_long.bin", None, 1), ("g1_edge.bin", None, 1), ("salmon_zero.bin", None, 1)]
GOLDEN_IDS = ["%s-s%s-m%d" % (f[:-4], "A" if s is None else s, mc) for f, s, mc in GOLDENS]
LITERALS = {("g2_c1.bin", None, 1): (40, 3313, 416, 25), ("g2_c1.bin", None, 2): (580, 1278, 131, 65), ("gt_h8.out.bin", None, 1): (1175, 2637, 2826, 1)}


def _want(name, sample, mc):
    return _kept.setdefault(("want", name, sample, mc), cc.components(*args_of(load(name)), sample=sample, min_count=mc))


def _file_text(m, of_locus, multi_only=False):
    """The cluster file written out from the definition: a line per component, its first target's name, then all its targets."""
    lines = {}
    for t, c in enumerate(of_locus):
        lines.setdefault(int(c), []).append(m.lname[t])
    return "".join("\t".join([v[0]] + v) + "\n" for c, v in sorted(lines.items()) if len(v) >= (2 if multi_only else 1))


def _stats_text(want, multi_only=False):
    rows = [(c, int(want[2][c]), int(want[3][c]), int(want[4][c])) for c in range(want[5][0]) if want[2][c] >= (2 if multi_only else 1)]
    return "cluster\ttargets\tecs\treads\n" + "".join("%d\t%d\t%d\t%d\n" % r for r in rows)


@pytest.mark.parametrize("name,sample,mc", GOLDENS, ids=GOLDEN_IDS)
def test_goldens_through_the_binding_on_arrays_and_on_tensors(name, sample, mc):
    want = _want(name, sample, mc)
    if (name, sample, mc) in LITERALS:
        assert want[5] == LITERALS[(name, sample, mc)]
    for tensors in (False, True):
        _same(_run(args_of(load(name)), tensors=tensors, sample=sample, min_count=mc), want, tensors)


@pytest.mark.parametrize("name,sample,mc", GOLDENS, ids=GOLDEN_IDS)
def test_goldens_through_the_file_command(name, sample, mc, tmp_path):
    m, want = load(name), _want(name, sample, mc)
    out, stats = str(tmp_path / "c.grp.txt"), str(tmp_path / "stats.tsv")
    for multi_only in (False, True):
        bin_utils.ecclusters(os.path.join(GOLDEN, name), out, sample=None if sample is None else m.sname[sample], min_count=mc, stats_file=stats,
                             multi_only=multi_only)
        assert open(out).read() == _file_text(m, want[0], multi_only) and open(stats).read() == _stats_text(want, multi_only)
    gene, _ = bin_utils.gene_ids(m, out)                               # (the --multi-only file: the same partition)
    assert len(set(zip(gene.tolist(), want[0].tolist()))) == want[5][0]


def test_goldens_through_the_command_line(tmp_path):
    env = dict(os.environ)
    env.pop("ALNTOOLS_GPUS", None)
    env["ALNTOOLS_TORCH"] = "0"

    def cli(*argv):
        return subprocess.run([sys.executable, "-m", "alntools_amd.cli", "ecclusters"] + list(argv), cwd=ROOT, env=env, capture_output=True, text=True,
                              timeout=300)
    out, stats = str(tmp_path / "c.grp.txt"), str(tmp_path / "stats.tsv")
    m, want = load("g2_c1.bin"), _want("g2_c1.bin", None, 2)
    r = cli(os.path.join(GOLDEN, "g2_c1.bin"), out, "-m", "2", "--stats", stats, "-v")
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(out).read() == _file_text(m, want[0]) and open(stats).read() == _stats_text(want)
    assert "Number of clusters: 580 (65 of two targets or more), from 1,278 linking ECs" in r.stderr and "Largest cluster: 131 targets" in r.stderr
    m, want = load("gt_ms.out.bin"), _want("gt_ms.out.bin", 5, 1)
    r = cli(os.path.join(GOLDEN, "gt_ms.out.bin"), out, "-s", m.sname[5], "--multi-only", "--stats", stats)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(out).read() == _file_text(m, want[0], True) and open(stats).read() == _stats_text(want, True)
    r = cli(os.path.join(GOLDEN, "gt_ms.out.bin"), out + "2", "-s", "NOPE")
    assert r.returncode == 1 and "Error: sample NOPE is not in" in r.stderr and not os.path.exists(out + "2")
    r = cli(os.path.join(GOLDEN, "gt_ms.out.bin"), out + "2", "-m", "-1")
    assert r.returncode == 1 and "Error: the minimum count" in r.stderr and not os.path.exists(out + "2")


# ---- the shapes at which a concurrent union-find goes wrong ---------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_a_chain_in_three_row_orders(order):
    T = 4097
    t = np.arange(T - 1)
    k = {"ascending": t, "descending": t[::-1].copy(), "shuffled": np.random.default_rng(1).permutation(T - 1)}[order]
    want = _check(_pairs(t, t + 1, T, order=k), order)
    assert want[5] == (1, T - 1, T, 1)


@pytest.mark.parametrize("centre", ["first", "last"])
def test_a_star_whose_centre_is_the_smallest_or_the_largest_locus(centre):
    """8192 rows {0, t}; and {t, T - 1}, where the root has to move every time a smaller locus joins."""
    T = 8193
    t = np.arange(1, T) if centre == "first" else np.arange(T - 1)
    c = np.zeros(T - 1, dtype=np.int64) if centre == "first" else np.full(T - 1, T - 1)
    want = _check(_pairs(t, c, T, order=np.random.default_rng(2).permutation(T - 1) if centre == "last" else None), centre)
    assert want[5] == (1, 8192, T, 1)


def test_ten_thousand_copies_of_one_row():
    want = _check(_csr([[3, 17, 40, 99]] * 10000, 128))
    assert want[5] == (125, 10000, 4, 1) and int(want[4][3]) == 10000


def test_two_halves_that_only_the_last_row_joins():
    h = 2048
    t = np.concatenate([np.arange(h - 1), np.arange(h, 2 * h - 1)])
    a = np.concatenate([t, [h - 1]])
    want = _check(_pairs(a, a + 1, 2 * h))
    assert want[5] == (1, 2 * h - 1, 2 * h, 1)
    assert cc.components(*_pairs(t, t + 1, 2 * h))[5][0] == 2


def test_rounds_of_pairwise_merges_make_deep_trees():
    """Round k joins blocks of 2^k loci in pairs, by one row between a random locus of each: 12 rounds over 4096 loci, the rows in round
    order and shuffled."""
    T, rng = 4096, np.random.default_rng(3)
    a, b = [], []
    for k in range(12):
        left = np.arange(0, T, 2 << k)
        a.append(left + rng.integers(0, 1 << k, size=len(left)))
        b.append(left + (1 << k) + rng.integers(0, 1 << k, size=len(left)))
    a, b = np.concatenate(a), np.concatenate(b)
    for order in (None, rng.permutation(len(a)), np.arange(len(a))[::-1].copy()):
        assert _check(_pairs(a, b, T, order=order))[5] == (1, T - 1, T, 1)
    assert _check(_pairs(a[:-1], b[:-1], T))[5][0] == 2                 # (without the last round's row: two halves)


def test_one_row_of_every_locus_among_rows_of_one():
    T = 5000
    rows = [[t] for t in range(0, T, 2)] + [list(range(T))] + [[t] for t in range(1, T, 2)]
    want = _check(_csr(rows, T))
    assert want[5] == (1, T + 1, T, 1)
    assert _check(_csr(rows, T, N=(np.array([0, T], dtype=np.int32), np.delete(np.arange(T + 1), T // 2).astype(np.int32), np.ones(T, dtype=np.int32))),
                  "the long row weighs nothing")[5] == (T, T, 1, 0)


@pytest.mark.parametrize("length", [CC_ITEMS - 1, CC_ITEMS, CC_ITEMS + 1, CC_WG_ITEMS - 1, CC_WG_ITEMS, CC_WG_ITEMS + 1, 2 * CC_WG_ITEMS + 1])
def test_row_lengths_around_a_threads_and_a_workgroups_items(length):
    """A row of ``length`` loci at every residue modulo CC_ITEMS of its first non-zero, pairs before and after it."""
    T = 2 * length + 64
    rng = np.random.default_rng(length)
    for shift in range(CC_ITEMS):
        long = np.sort(rng.choice(T - 32, size=length, replace=False)).tolist()
        rows = [[T - 32 + 2 * k, T - 31 + 2 * k] for k in range(3)] + [[T - 20 + k] for k in range(shift)] + [long] + [[T - 10, T - 9], [T - 9, T - 8]]
        want = _check(_csr(rows, T), (length, shift))
        assert want[2][want[0][long[0]]] == length and want[5][3] == 5


@pytest.mark.parametrize("share", [4, 2, 1], ids=["E=T/4", "E=T/2", "E=T"])
def test_random_rows_below_at_and_above_the_giant_component(share):
    T, rng = 20000, np.random.default_rng(40 + share)
    E = T // share
    lens = 1 + rng.poisson(2, size=E)
    ip = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    key = np.repeat(np.arange(E, dtype=np.int64), lens) * T + rng.integers(0, T, size=int(ip[-1]))
    key = np.unique(key)                                                # (a locus twice in a row: once)
    row = key // T
    ip = np.searchsorted(row, np.arange(E + 1)).astype(np.int32)
    ix = (key % T).astype(np.int32)
    da = rng.integers(1, 4, size=len(ix)).astype(np.int32)
    xn = np.flatnonzero(rng.random(E) < 0.9).astype(np.int32)
    N = (np.array([0, len(xn)], dtype=np.int32), xn, rng.integers(0, 5, size=len(xn)).astype(np.int32))
    assert len(ix) <= 200000
    for mc in (1, 3):
        want = _check((ip, ix, da, T, 2) + N, (share, mc), min_count=mc)
        print("E = T / %d, min_count %d: %d components, the largest of %d loci" % (share, mc, want[5][0], want[5][2]))
    if share == 1:                                                      # (E = T: a giant component)
        assert cc.components(*((ip, ix, da, T, 2) + N))[5][2] > T // 4


# ---- masks of 0 ------------------------------------------------------------------------------------------------------------------------------
def test_a_mask_of_zero_is_no_member():
    rows = [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10], [11, 12], [12, 13], [14, 15, 16, 17, 18], [19]]
    masks = [[0, 1, 1], [1, 0, 1], [1, 1, 0], [0, 0], [1, 0], [0, 1], [0, 1, 0, 0, 1], [0]]
    want = _check(_csr(rows, 20, masks=masks))
    loc, ec = want[0], want[1]
    assert loc[0] != loc[1] == loc[2]                                   # first in a row
    assert loc[3] == loc[5] != loc[4]                                   # in the middle: the members on both sides of it are still joined
    assert loc[6] == loc[7] != loc[8]                                   # last
    assert ec[3] == -1 and ec[7] == -1 and loc[9] != loc[10]            # a row of nothing else links nothing
    assert len({loc[11], loc[12], loc[13]}) == 3                        # two loci that only a zero-mask entry would tie
    assert loc[15] == loc[18] and len({loc[14], loc[16], loc[17], loc[15]}) == 4
    assert ec[0] == loc[1] and ec[4] == loc[11] and ec[5] == loc[13] and want[5] == (16, 6, 2, 4)


@pytest.mark.parametrize("zeros", [0.02, 0.5, 0.97])
def test_random_rows_with_masks_of_zero(zeros):
    rng = np.random.default_rng(int(zeros * 100))
    T, E = 3000, 4000
    lens = rng.integers(0, 12, size=E)
    lens[7], lens[2000] = CC_WG_ITEMS + 3, 2 * CC_WG_ITEMS
    rows = [np.sort(rng.choice(T, size=int(n), replace=False)).tolist() for n in lens]
    masks = [np.where(rng.random(len(r)) < zeros, 0, rng.integers(1, 8, size=len(r))).tolist() for r in rows]
    a = _csr(rows, T, H=3, masks=masks)
    assert (a[2] == 0).any() and (a[2] != 0).any()
    for mc in (0, 1):
        _check(a, zeros, min_count=mc)


# ---- weights ---------------------------------------------------------------------------------------------------------------------------------
def test_weights_decide_which_rows_link():
    rng = np.random.default_rng(8)
    ip, ix, da = gt_checker.random_csr(rng, 3000, 900, 4, max_row=60)
    E = 3000
    # three samples: ECs N does not list, counts of 0, an EC listed twice more in a column (its counts add up to the threshold)
    cols = [np.sort(rng.choice(E, size=k, replace=False)) for k in (1500, 40, 2200)]
    twice = int(next(e for e in cols[1] if ip[e + 1] - ip[e] >= 2))
    cols[1] = np.concatenate([cols[1], [twice, twice]])
    pn = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    xn = np.concatenate(cols).astype(np.int32)
    dn = rng.integers(0, 4, size=len(xn)).astype(np.int32)
    dn[pn[1]:pn[2]] = 1
    a = (ip, ix, da, 900, 4, pn, xn, dn)
    for sample in (None, 0, 1, 2):
        for mc in (0, 1, 2, 3, 7):
            want = _check(a, (sample, mc), sample=sample, min_count=mc)
            if mc == 0:
                assert want[5][1] == int((np.diff(ip) > 0).sum())      # every row with a member links
    assert cc.components(*a, sample=1, min_count=3)[1][twice] >= 0 and cc.components(*a, sample=1, min_count=3)[5][1] == 1
    assert cc.components(*a, sample=1, min_count=4)[5] == (900, 0, 1, 0)


# ---- degenerate inputs -----------------------------------------------------------------------------------------------------------------------
def test_degenerate_inputs():
    none = (np.array([0, 0], dtype=np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))      # (one sample, no entry)
    assert _check((np.array([0], dtype=np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), 5, 2) + none, "E = 0")[5] == (5, 0, 1, 0)
    assert _check(_csr([[], [], [], []], 7), "nnz = 0")[5] == (7, 0, 1, 0)
    assert _check(_csr([[0], [0]], 1), "T = 1")[5] == (1, 2, 1, 0)
    assert _check(_csr([[]], 1), "T = 1, nothing")[5] == (1, 0, 1, 0)
    want = _check(_csr([[t % 50] for t in range(3000)], 64), "rows of one")
    assert want[5] == (64, 3000, 1, 0) and int(want[3][7]) == 60 and int(want[3][63]) == 0


# ---- one rule for every route ----------------------------------------------------------------------------------------------------------------
def _blob(out):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in out[:5]) + repr(tuple(out[5])).encode()


def _route_inputs():
    rng = np.random.default_rng(77)
    rows = [np.sort(rng.choice(5000, size=int(n), replace=False)).tolist() for n in np.minimum(1 + rng.poisson(1.2, size=6000), 9)]
    masks = [np.where(rng.random(len(r)) < 0.1, 0, 1).tolist() for r in rows]
    m = load("gt_h8.out.bin")
    return [(args_of(m), {}), (args_of(load("gt_ms.out.bin")), {"sample": 5}), (_csr(rows, 5000), {"min_count": 1}), (_csr(rows, 5000, masks=masks), {})]


def _routes():
    """Every input by both entry points, twice; asserts that the routes agree; -> one blob."""
    out = b""
    for a, kw in _route_inputs():
        first = _blob(_run(a, **kw))
        for tensors in (True, False, True):
            assert _blob(_run(a, tensors=tensors, **kw)) == first, (kw, tensors)
        out += first
    return out


def test_both_entry_points_and_a_second_call_give_the_same_bytes():
    first = _routes()
    assert first == b"".join(_blob(cc.components(*a, **kw)) for a, kw in _route_inputs())
    _kept["digest"] = hashlib.sha256(first).hexdigest()


def test_everything_once_more_with_the_scratch_poisoned_gives_the_same_bytes():
    if "digest" not in _kept:
        _kept["digest"] = hashlib.sha256(_routes()).hexdigest()
    env = dict(os.environ)
    env["ECB_POISON_SCRATCH"] = "1"
    env["ALNTOOLS_TORCH"] = "1"
    code = ("import sys, hashlib; sys.path[:0] = [%r, %r]; import test_gpu_ecclusters as t; print('digest', hashlib.sha256(t._routes()).hexdigest())"
            % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "digest " + _kept["digest"] in r.stdout


# ---- the contract ----------------------------------------------------------------------------------------------------------------------------
def test_contract_violations_leave_the_outputs_untouched_and_the_next_call_works():
    import torch
    lib = ecb_components.load()
    rng = np.random.default_rng(5)
    E, T, H = 3000, 500, 4
    ip, ix, da = gt_checker.random_csr(rng, E, T, H)
    pn = np.array([0, 1000, 1000, 2500], dtype=np.int32)
    xn = np.concatenate([np.sort(rng.choice(E, size=k, replace=False)) for k in (1000, 0, 1500)]).astype(np.int32)
    dn = rng.integers(0, 90, size=2500).astype(np.int32)
    good = cc.components(ip, ix, da, T, H, pn, xn, dn)
    a = int(ip[int(np.argmax(np.diff(ip)))])
    ok = dict(ip=ip, ix=ix, da=da, pn=pn, xn=xn, dn=dn, sample=-1, min_count=1)
    bad = []

    def breach(what, code=CONTRACT, **kw):
        bad.append((what, code, dict(ok, **kw)))

    p = ip.copy(); p[0] = 1; breach("indptr[0] != 0", ip=p)
    p = ip.copy(); p[-1] -= 1; breach("indptr[E] != nnz", ip=p)
    p = ip.copy(); p[10], p[11] = p[11] + 1, p[10]; breach("falling indptr", ip=p)
    p = ip.copy(); p[20] = len(ix) + 5; breach("indptr beyond nnz", ip=p)
    x = ix.copy(); x[5] = T; breach("locus >= T", ix=x)
    x = ix.copy(); x[7] = -1; breach("negative locus", ix=x)
    x = ix.copy(); x[a + 1], x[a + 2] = x[a + 2], x[a + 1]; breach("unsorted column", ix=x)
    x = ix.copy(); x[a + 2] = x[a + 1]; breach("duplicate column", ix=x)
    d = da.copy(); d[9] = 1 << H; breach("bit >= H", da=d)
    p = pn.copy(); p[0] = 1; breach("N pointers not from 0", pn=p)
    p = pn.copy(); p[-1] = 2499; breach("N pointers not to nnz_n", pn=p)
    p = pn.copy(); p[1], p[2] = 1200, 1100; breach("N pointers falling", pn=p)
    x = xn.copy(); x[3] = E; breach("EC >= n_ecs", xn=x)
    x = xn.copy(); x[4] = -2; breach("negative EC", xn=x)
    d = dn.copy(); d[2400] = -1; breach("negative count", dn=d)
    breach("sample = n_samples", sample=3)
    breach("sample = -2", sample=-2)
    breach("min_count = -1", code=ARG, min_count=-1)
    shapes = [(T,), (E,), (T,), (T,), (T,)]

    def call(k, host):
        arrs = [np.ascontiguousarray(k[n], dtype=np.int32) for n in ("ip", "ix", "da", "pn", "xn", "dn")]
        sizes = (C.c_uint64 * 4)(7, 7, 7, 7)
        if host:
            outs = [np.full(s, 7, dt) for s, dt in zip(shapes, DTYPES)]
            ptr = lambda v: v.ctypes.data_as(C.c_void_p)   # noqa: E731
            fn = lib.ecb_components
        else:
            arrs = [torch.from_numpy(v).cuda() for v in arrs]
            outs = [torch.full(s, 7, dtype=torch.int64 if dt == np.int64 else torch.int32, device="cuda") for s, dt in zip(shapes, DTYPES)]
            ptr = lambda v: C.c_void_p(v.data_ptr())       # noqa: E731
            fn = lib.ecb_components_device
        rc = fn(0, E, T, H, len(ix), ptr(arrs[0]), ptr(arrs[1]), ptr(arrs[2]), 3, len(xn), ptr(arrs[3]), ptr(arrs[4]), ptr(arrs[5]), k["sample"],
                k["min_count"], *([ptr(o) for o in outs] + [sizes]))
        return rc, [_np(o) for o in outs], tuple(sizes)

    for host in (False, True):
        for what, code, k in bad:
            rc, outs, sizes = call(k, host)
            assert rc == code, (what, host, rc, lib.ecb_last_error(None))
            assert all((o == 7).all() for o in outs) and sizes == (7, 7, 7, 7), (what, host)
            rc, outs, sizes = call(ok, host)                           # the device is unharmed
            assert rc == 0, (what, host)
            C_ = good[5][0]
            assert not any(o[C_:].any() for o in outs[2:])              # all T entries written: 0 at and beyond C
            _same(outs[:2] + [o[:C_] for o in outs[2:]] + [sizes], good, what)


def test_null_outputs_are_skipped():
    lib = ecb_components.load()
    m = load("g2_c1.bin")
    want = _want("g2_c1.bin", None, 1)
    arrs = [np.ascontiguousarray(v, dtype=np.int32) for v in (m.indptrA, m.indicesA, m.dataA, m.indptrN, m.indicesN, m.dataN)]
    ptr = lambda v: v.ctypes.data_as(C.c_void_p)   # noqa: E731
    of_locus, reads = np.full(m.num_loci, 7, np.int32), np.full(m.num_loci, 7, np.int64)
    sizes = (C.c_uint64 * 4)()
    rc = lib.ecb_components(0, m.num_reads, m.num_loci, m.num_haplotypes, len(arrs[1]), ptr(arrs[0]), ptr(arrs[1]), ptr(arrs[2]), 1, len(arrs[4]),
                            ptr(arrs[3]), ptr(arrs[4]), ptr(arrs[5]), -1, 1, ptr(of_locus), None, None, None, ptr(reads), sizes)
    assert rc == 0 and tuple(sizes) == want[5] and np.array_equal(of_locus, want[0])
    assert np.array_equal(reads[:want[5][0]], want[4]) and not reads[want[5][0]:].any()


# ---- the cluster file does what it is for ------------------------------------------------------------------------------------------------------
def test_bundling_by_the_default_cluster_file_leaves_every_read_with_one_target(tmp_path):
    src = os.path.join(GOLDEN, "g2_c1.bin")
    grp, out = str(tmp_path / "c.grp.txt"), str(tmp_path / "bundled.bin")
    bin_utils.ecclusters(src, grp)
    bin_utils.ecbundle(src, grp, out)
    m, b = load("g2_c1.bin"), bin_utils.ecload(out)
    assert b.num_loci == _want("g2_c1.bin", None, 1)[5][0] == 40
    lu = ecb.count_alignments(*args_of(b))[2]
    assert int(lu.sum()) == int(b.dataN.sum()) == int(m.dataN.sum())    # every read is locus-unique, and none was lost
    assert int(np.diff(b.indptrA).max()) == 1                          # no EC has two targets
