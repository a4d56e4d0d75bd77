"""ecquant per cell on the GPU (``ecb_cell_support*`` / ``ecb_quantify_cells*``) against the step pairs recorded from the reference and against
the cell checker (``tests/cell_quant_checker.py``): every recorded pair through both entry points, theta_0 and the support, every cell's own
stop, one rule for every route (two calls, both entries, every batching, a cell alone, the merged ``ecb.quantify(sample=c)``, all of it once
more with the scratch poisoned), the paths' edges, many workgroups, every refusal with its outputs untouched, the empty inputs and the command.

The tolerance of one step of one cell is derived in ``test_ecquant.py``: (B + L + 4) 2^-52 relative with the cell's own B and L, entry by
entry, the same entries 0.  The E-step's split of a row (per non-zero, then per row) adds no rounding: every partial sum starts from an exact
0, so a row of B set bits still takes B - 1 rounded additions."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from alntools_amd import bin_utils, ecb

import cell_quant_checker as cq
import counts_checker
import quant_checker as qchk
from test_ecquant_cells import MS, QC_LONG_COL, QC_LONG_ROW, QC_TILE, RECORDED, TPB, ms, npz
from test_quant_constants import Q_BATCH

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
INFO = ("n_iter", "delta", "explained", "converged")
_kept_bytes = {}


def _names(n, p):
    return ["%s%d" % (p, i) for i in range(n)]


def _mat(H, T, indptrA, indicesA, dataA, indptrN, indicesN, dataN):
    S = len(indptrN) - 1
    return bin_utils.ECMatrices(_names(H, "h"), _names(T, "t"), np.ones((T, H)), _names(S, "s"), indptrA, indicesA, dataA, indptrN, indicesN, dataN)


def _args(m, tensors):
    a = [m.indptrA, m.indicesA, m.dataA, m.indptrN, m.indicesN, m.dataN]
    if tensors:
        import torch
        a = [torch.as_tensor(np.asarray(x, dtype=np.int32), device="cuda") for x in a]
    return a[0], a[1], a[2], m.num_loci, m.num_haplotypes, a[3], a[4], a[5]


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def _qc(m, tensors=False, cell_keep=None, scale=None, theta_in=None, **kw):
    """ecb.quantify_cells over an ECMatrices -> (cell_ptr, slot_locus, theta, info) as numpy, through the host entry or, with CUDA tensors, the
    device entry."""
    if tensors:
        import torch
        scale, theta_in = (None if t is None else torch.as_tensor(np.asarray(t, dtype=np.float64), device="cuda") for t in (scale, theta_in))
    ptr, loc, theta, info = ecb.quantify_cells(*_args(m, tensors), cell_keep=cell_keep, scale=scale, theta_in=theta_in, **kw)
    if tensors:
        assert ptr.is_cuda and loc.is_cuda and theta.is_cuda and all(info[k].is_cuda for k in INFO)
    ptr, loc, theta = _np(ptr), _np(loc), _np(theta)
    info = {k: _np(info[k]) for k in INFO}
    S = m.num_samples
    assert ptr.shape == (S + 1,) and ptr.dtype == np.int64 and loc.dtype == np.int32 and theta.dtype == np.float64
    assert theta.shape == (len(loc), m.num_haplotypes) and ptr[0] == 0 and ptr[-1] == len(loc) and all(info[k].shape == (S,) for k in INFO)
    return ptr, loc, theta, info


def _blob(res):
    ptr, loc, theta, info = res
    return ptr.tobytes() + loc.tobytes() + theta.tobytes() + b"".join(np.ascontiguousarray(info[k]).astype(np.float64).tobytes() for k in INFO)


def _cell_blob(res, c):
    ptr, loc, theta, info = res
    a, b = int(ptr[c]), int(ptr[c + 1])
    return loc[a:b].tobytes() + theta[a:b].tobytes() + b"".join(np.float64(info[k][c]).tobytes() for k in INFO)


# ---- 1. the recorded pairs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,k,file,pre", RECORDED, ids=["cell%d-k%d" % r[:2] for r in RECORDED])
def test_every_recorded_pair_through_both_entry_points(c, k, file, pre):
    m, cs = ms()
    z = npz(file)
    cell, ref = cs[c], z[pre + "next_%d" % k]
    for tensors in (False, True):
        ptr, loc, theta, info = _qc(m, tensors, theta_in=z[pre + "theta_%d" % k], max_iters=1, tol=0.0)       # all 338 cells from this cell's theta_k
        got = cell.scatter(theta[ptr[c]:ptr[c + 1]])
        worst = qchk.agree(got, ref, cell.tolerance())
        print("cell %d k=%d %s: worst relative difference %.3g, bound %.3g" % (c, k, "device" if tensors else "host", worst, cell.tolerance()))
        assert np.array_equal(loc[ptr[c]:ptr[c + 1]], cell.support) and info["n_iter"][c] == 1 and info["explained"][c] == cell.W
        assert abs(float(got.sum()) - cell.W) <= cell.tolerance() * cell.W


# ---- 2. theta_0 and the support -----------------------------------------------------------------------------------------------------------
def test_theta_0_is_each_cells_aln_and_the_support_is_where_it_is_positive():
    m, cs = ms()
    a = (m.indptrA, m.indicesA, m.dataA, m.num_loci, m.num_haplotypes, m.indptrN, m.indicesN, m.dataN)
    alns = [counts_checker.count(*a, sample=c)[0] for c in range(m.num_samples)]
    want_ptr = np.concatenate([[0], np.cumsum([int((x.sum(axis=0) > 0).sum()) for x in alns])])
    want_loc = np.concatenate([np.flatnonzero(x.sum(axis=0) > 0) for x in alns])
    assert np.array_equal(alns[0], npz("quant_ms_s0.npz")["theta_0"])
    for tensors in (False, True):
        ptr, loc, theta, info = _qc(m, tensors, max_iters=0)
        assert np.array_equal(ptr, want_ptr) and np.array_equal(loc, want_loc)
        for c, x in enumerate(alns):
            assert np.array_equal(theta[ptr[c]:ptr[c + 1]], x[:, loc[ptr[c]:ptr[c + 1]]].T), c
        assert (theta.max(axis=1) > 0).all()                            # every slot has an entry > 0
        assert not info["explained"].any() and not info["n_iter"].any() and not info["delta"].any() and info["converged"].all()
        sp, sl = ecb.cell_support(*_args(m, tensors))
        assert np.array_equal(_np(sp), want_ptr) and np.array_equal(_np(sl), want_loc) and _np(sl).dtype == np.int32
    keep = np.zeros(m.num_samples, dtype=bool)
    keep[[0, 3, 337]] = True
    sp, sl = ecb.cell_support(*_args(m, False), cell_keep=keep)
    assert np.array_equal(np.diff(sp), np.diff(want_ptr) * keep) and np.array_equal(sl, np.concatenate([cs[c].support for c in (0, 3, 337)]))


# ---- 3. independent stops -----------------------------------------------------------------------------------------------------------------
TOL, ITERS = 1e-6, 300


def _checker_runs():
    """Every cell's own run by the checker, once: [(theta, info)]."""
    if "runs" not in _kept_bytes:
        _kept_bytes["runs"] = [c.run(max_iters=ITERS, tol=TOL) for c in ms()[1]]
    return _kept_bytes["runs"]


def test_every_cell_stops_at_its_own_step():
    m, cs = ms()
    runs = _checker_runs()
    n = np.array([i["n_iter"] for _, i in runs])
    conv = np.array([i["converged"] for _, i in runs])
    ratio = np.array([i["delta"] / (TOL * c.W) for c, (_, i) in zip(cs, runs) if i["n_iter"]])
    # the spread the checker computes, asserted before the device is looked at
    assert len(set(n.tolist())) == 118 and int((n == 1).sum()) == 78 and int((~conv).sum()) == 28 and int((n > 2 * Q_BATCH).sum()) == 241
    closest = ratio[np.argmin(np.abs(ratio - 1.0))]
    assert abs(closest - 0.99977) < 5e-6, closest
    res = {}
    for tensors in (False, True):
        res[tensors] = ptr, loc, theta, info = _qc(m, tensors, max_iters=ITERS, tol=TOL)
        for c, (cell, (_, ri)) in enumerate(zip(cs, runs)):
            k = int(info["n_iter"][c])
            at = ri if k == ri["n_iter"] else cell.run(max_iters=k, tol=0.0)[1]        # (the checker's figures at the device's step)
            bound = cell.tolerance() * max(k, 1)
            assert abs(k - ri["n_iter"]) <= 1, (c, k, ri["n_iter"])
            if bool(info["converged"][c]) != ri["converged"]:           # only within one step of the stop: the last step allowed, or the one after it
                assert ri["n_iter"] >= ITERS - 1 if ri["converged"] else cell.run(max_iters=ITERS + 1, tol=TOL)[1]["converged"], c
            if info["converged"][c]:
                assert info["delta"][c] <= TOL * cell.W
            else:
                assert k == ITERS, (c, k)
            assert abs(info["delta"][c] - at["delta"]) <= bound * at["explained"], c
            assert abs(int(info["explained"][c]) - at["explained"]) <= bound * at["explained"], c
    assert _blob(res[False]) == _blob(res[True])
    # one late cell, two steps short: unconverged exactly there; its neighbours stop where they did
    late = int(np.flatnonzero(conv & (n > 2 * Q_BATCH + 2))[-1])
    nd = int(res[False][3]["n_iter"][late])                             # (the device's own step for it)
    short = _qc(m, max_iters=nd - 2, tol=TOL)
    assert short[3]["n_iter"][late] == nd - 2 and not short[3]["converged"][late] and short[3]["delta"][late] > TOL * cs[late].W
    early = np.flatnonzero(res[False][3]["n_iter"] < nd - 2)
    assert len(early) > 50 and all(_cell_blob(short, c) == _cell_blob(res[False], c) for c in early)


# ---- 4. one rule for every route ----------------------------------------------------------------------------------------------------------
def _routes():
    """The full run by every route; -> the bytes all of them gave."""
    m, cs = ms()
    kw = dict(max_iters=2 * Q_BATCH + 3, tol=1e-4)                      # (some cells stop early, some run out of steps)
    first = _qc(m, **kw)
    blob = _blob(first)
    assert 0 < first[3]["converged"].sum() < m.num_samples
    x = np.array([c.row_len.sum() for c in cs])
    per_x = 64 + 4 * 8 * m.num_haplotypes                               # (QC_X_BYTES + QC_SLOT_TABLES x 8 H: a batch holds budget / this)
    for tensors, more in ((False, {}), (True, {}), (False, dict(budget_bytes=1)), (True, dict(budget_bytes=1)),
                          (False, dict(budget_bytes=int(x.sum() // 5 + 1) * per_x)), (True, dict(budget_bytes=int(x.sum() // 3) * per_x)),
                          (True, dict(budget_bytes=0))):
        assert _blob(_qc(m, tensors, **dict(kw, **more))) == blob, (tensors, more)
    assert x.max() < x.sum() // 5                                       # (those budgets cut a handful of batches, none of one cell)
    theta_in = npz("quant_ms_s0.npz")["theta_5"]
    one = _qc(m, theta_in=theta_in, max_iters=1, tol=0.0)
    for c in (0, m.num_samples - 1, int(np.argmax(x))):                 # first, last, largest
        keep = np.zeros(m.num_samples, dtype=np.uint8)
        keep[c] = 1
        for tensors in (False, True):
            alone = _qc(m, tensors, cell_keep=keep, **kw)
            assert _cell_blob(alone, c) == _cell_blob(first, c) and alone[0][-1] == len(cs[c].support)
            assert alone[3]["converged"][np.arange(m.num_samples) != c].all() and not alone[3]["n_iter"][np.arange(m.num_samples) != c].any()
        # the merged, reference-pinned code on the same cell
        ref, rinfo = ecb.quantify(m.indptrA, m.indicesA, m.dataA, m.num_loci, m.num_haplotypes, m.indptrN, m.indicesN, m.dataN, sample=c,
                                  theta_in=cs[c].scatter(cs[c].gather(theta_in)), max_iters=1, tol=0.0)
        got = cs[c].scatter(one[2][one[0][c]:one[0][c + 1]])
        qchk.agree(got, ref, cs[c].tolerance())                         # (the bound is that of two computed results)
        assert rinfo["explained"] == one[3]["explained"][c]
        blob += got.tobytes()
    return blob


def test_one_rule_for_every_route():
    _kept_bytes["routes"] = _routes()


def _digest():
    h = hashlib.sha256()
    for key, make in [("routes", _routes)] + [("edge%d" % H, lambda H=H: _edge_case(H)) for H in EDGE_H]:
        if key not in _kept_bytes:
            _kept_bytes[key] = make()
        h.update(_kept_bytes[key])
    return h.hexdigest()


def test_everything_once_more_with_the_scratch_poisoned_gives_the_same_bits():
    """One child process with ECB_POISON_SCRATCH=1 repeats the routes and the edge cases: every buffer the library allocates is filled with
    0x01 first, so a pass that relied on fresh memory being 0 gives other bits than this process."""
    env = dict(os.environ)
    env["ECB_POISON_SCRATCH"] = "1"
    env["ALNTOOLS_TORCH"] = "1"
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_ecquant_cells as t; print('digest', t._digest())" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "digest " + _digest() in r.stdout


# ---- 5. the paths' edges ------------------------------------------------------------------------------------------------------------------
EDGE_H = [1, 2, 8, 31]
EDGE_T = 700
EDGE_CELLS = ("empty_first", "random", "zero_counts", "zero_masks", "one_entry", "twice", "empty_middle", "long_rows", "long_cols", "chunk_lo",
              "chunk_at", "chunk_hi", "random2", "empty_last")


def _edge_matrix(H, seed=31):
    """Seeded.  Rows of A: 400 random ones over the loci from 3 on (loci 0, 1 and 2 added to the first QC_LONG_COL - 1, QC_LONG_COL and
    QC_LONG_COL + 1 of them, with masks other than 0); a row of stored zeros; rows of QC_LONG_ROW - 1, QC_LONG_ROW and QC_LONG_ROW + 1
    non-zeros; rows of TPB / H - 1, TPB / H and TPB / H + 1 non-zeros without a stored 0.  The cells: EDGE_CELLS."""
    rng = np.random.default_rng(seed + H)
    T, n_rand = EDGE_T, 400
    rows = []
    for e in range(n_rand):
        cols = np.sort(rng.choice(np.arange(3, T), size=int(rng.integers(0, 9)), replace=False))
        lead = np.array([c for c, k in ((0, QC_LONG_COL - 1), (1, QC_LONG_COL), (2, QC_LONG_COL + 1)) if e < k], dtype=np.int64)
        masks = rng.integers(1, 1 << H, size=len(lead) + len(cols), dtype=np.int64)
        masks[len(lead):][rng.random(len(cols)) < 0.04] = 0             # stored masks of 0, never at the leading loci
        rows.append((np.concatenate([lead, cols]), masks))
    special = {}
    def add(name, cols, masks):
        special[name] = len(rows)
        rows.append((np.sort(cols), masks))
    add("zeros", rng.choice(np.arange(3, T), size=5, replace=False), np.zeros(5, dtype=np.int64))
    for n in (QC_LONG_ROW - 1, QC_LONG_ROW, QC_LONG_ROW + 1):
        add("row%d" % n, rng.choice(np.arange(3, T), size=n, replace=False), rng.integers(1, 1 << H, size=n, dtype=np.int64))
    k = TPB // H
    for name, n in (("chunk_lo", k - 1), ("chunk_at", k), ("chunk_hi", k + 1)):
        add(name, rng.choice(np.arange(3, T), size=n, replace=False), rng.integers(1, 1 << H, size=n, dtype=np.int64))
    indptr = np.cumsum([0] + [len(r[0]) for r in rows])
    indices = np.concatenate([r[0] for r in rows])
    data = np.concatenate([r[1] for r in rows])
    some = lambda n: np.sort(rng.choice(n_rand, size=n, replace=False))      # noqa: E731
    r1, r2 = some(60), some(90)
    cells = {"empty_first": ([], []), "random": (r1, rng.integers(1, 50, size=60)), "zero_counts": (some(7), np.zeros(7, dtype=np.int64)),
             "zero_masks": ([special["zeros"]], [4]), "one_entry": ([5], [3]),
             "twice": ([10, 11, 10, 300], [2, 5, 9, 0]), "empty_middle": ([], []),
             "long_rows": ([special["row%d" % n] for n in (QC_LONG_ROW - 1, QC_LONG_ROW, QC_LONG_ROW + 1)] + [7], [3, 1, 8, 2]),
             "long_cols": (np.arange(QC_LONG_COL + 1), rng.integers(1, 9, size=QC_LONG_COL + 1)),
             "chunk_lo": ([special["chunk_lo"]], [6]), "chunk_at": ([special["chunk_at"], special["chunk_at"]], [1, 2]),
             "chunk_hi": ([special["chunk_hi"]], [5]), "random2": (r2, rng.integers(0, 30, size=90)), "empty_last": ([], [])}
    assert tuple(cells) == EDGE_CELLS
    ipn = np.cumsum([0] + [len(cells[c][0]) for c in EDGE_CELLS])
    ixn = np.concatenate([np.asarray(cells[c][0], dtype=np.int64) for c in EDGE_CELLS])
    dn = np.concatenate([np.asarray(cells[c][1], dtype=np.int64) for c in EDGE_CELLS])
    m = _mat(H, T, indptr, indices, data, ipn, ixn, dn)
    theta_in = rng.random((H, T)) * 10 + 0.01
    has_bit = lambda e: e > QC_LONG_COL and bool(data[indptr[e]:indptr[e + 1]].any())      # noqa: E731
    dn2 = dn[ipn[12]:ipn[13]]
    for e in [e for e in r1 if has_bit(e)][:2] + [e for e, n in zip(r2, dn2) if n and has_bit(e) and e not in r1][:1]:
        theta_in[:, indices[indptr[e]:indptr[e + 1]]] = 0.0            # rows whose targets all have theta = 0: d = 0 wherever they are listed
    scale = 1.0 / rng.integers(1, 3000, size=(H, T))
    return m, theta_in, scale


def _edge_case(H):
    m, theta_in, scale = _edge_matrix(H)
    cs = cq.cells(m)
    by = dict(zip(EDGE_CELLS, cs))
    # the matrix really holds what it was built for
    assert all(by[c].empty() and len(by[c].rows) == 0 for c in ("empty_first", "empty_middle", "empty_last")) and cs[0].empty() and cs[-1].empty()
    assert by["zero_counts"].empty() and m.indptrN[3] - m.indptrN[2] == 7
    assert by["zero_masks"].empty() and len(by["zero_masks"].rows) == 1 and by["zero_masks"].row_len.tolist() == [5]
    assert len(by["one_entry"].rows) == 1 and not by["one_entry"].empty()
    tw = m.indicesN[m.indptrN[5]:m.indptrN[6]]
    assert tw.tolist().count(10) == 2 and len(by["twice"].rows) == 3
    assert by["long_rows"].row_len.tolist()[:3] == [QC_LONG_ROW - 1, QC_LONG_ROW, QC_LONG_ROW + 1]
    assert by["long_cols"].col_len[:3].tolist() == [QC_LONG_COL - 1, QC_LONG_COL, QC_LONG_COL + 1] and by["long_cols"].support[:3].tolist() == [0, 1, 2]
    items = [len(by[c].support) * H for c in ("chunk_lo", "chunk_at", "chunk_hi")]
    assert items == [(TPB // H - 1) * H, TPB // H * H, (TPB // H + 1) * H] and items[0] < TPB and items[1] <= TPB < items[2]
    assert H != 1 or items == [TPB - 1, TPB, TPB + 1]
    assert (m.dataA == 0).any() and (m.dataN == 0).any()
    # (the per-cell reduce has one level -- thread k adds parts k, k + TPB, ... -- so there is no cell above TPB^2 to build)
    out = b""
    for sc in (None, scale):
        steps = [c.step(theta_in, sc) for c in cs]
        assert sum(ex < c.W for c, (_, ex) in zip(cs, steps)) >= 2      # rows with a count and d = 0
        steps0 = [c.step(c.p.aln(), sc) for c in cs]
        for tensors in (False, True):
            for refs, res in ((steps, _qc(m, tensors, scale=sc, theta_in=theta_in, max_iters=1, tol=0.0)),
                              (steps0, _qc(m, tensors, scale=sc, max_iters=1, tol=0.0))):
                ptr, loc, theta, info = res
                assert np.array_equal(ptr, cq.expected_support(cs)[0]) and np.array_equal(loc, cq.expected_support(cs)[1])
                for c, (cell, (ref, ex)) in enumerate(zip(cs, refs)):
                    qchk.agree(cell.scatter(theta[ptr[c]:ptr[c + 1]]), ref, cell.tolerance())
                    assert info["explained"][c] == ex and info["n_iter"][c] == (0 if cell.empty() else 1), (EDGE_CELLS[c], tensors)
                    assert not cell.empty() or (info["converged"][c] and info["delta"][c] == 0)
                if refs is steps0:
                    assert all(info["explained"][c] == cell.W for c, cell in enumerate(cs))
                out += _blob(res)
    return out


@pytest.mark.parametrize("H", EDGE_H)
def test_edges(H):
    _kept_bytes["edge%d" % H] = _edge_case(H)


# ---- 6. many workgroups -------------------------------------------------------------------------------------------------------------------
def test_many_workgroups():
    rng = np.random.default_rng(177)
    E, T, H, S = 20000, 5000, 8, 64
    lens = rng.integers(0, 12, size=E)
    lens[123] = 2000                                                    # one long row
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = np.concatenate([np.sort(rng.choice(T, size=n, replace=False)) for n in lens])
    hot = rng.random(len(indices)) < 0.05                               # a few hot columns: 0, wherever the row does not hold it yet
    first = np.zeros(len(indices), dtype=bool)
    first[indptr[:-1][lens > 0]] = True
    indices[hot & first & (indices > 0)] = 0
    data = rng.integers(1, 1 << H, size=len(indices))
    sizes = np.concatenate([[0, 1, 3], rng.integers(10, 400, size=S - 9), [0, 2500, 4000, 6000, 1500, 0]])        # uneven: 0 to several thousand entries
    listed = [np.setdiff1d(rng.choice(E, size=n, replace=False), [123]) for n in sizes]
    for c in (5, 40, S - 3):                                            # the long row in three cells
        listed[c] = np.union1d(listed[c], [123])
    ipn = np.concatenate([[0], np.cumsum([len(x) for x in listed])])
    counts = rng.integers(0, 60, size=int(ipn[-1]))
    for c in (5, 40, S - 3):
        counts[ipn[c] + int(np.searchsorted(listed[c], 123))] = 7
    m = _mat(H, T, indptr, indices, data, ipn, np.concatenate(listed), counts)
    cs = cq.cells(m)
    assert sum(123 in m.indicesN[m.indptrN[c]:m.indptrN[c + 1]][m.dataN[m.indptrN[c]:m.indptrN[c + 1]] > 0] for c in range(S)) == 3
    assert max(c.col_len.max() for c in cs if not c.empty()) > QC_LONG_COL and max(c.row_len.sum() for c in cs) > 4 * QC_TILE
    assert sum(c.empty() for c in cs) >= 3 and max(len(c.rows) for c in cs) > 4000 and sum(len(c.support) for c in cs) * H > 100 * TPB
    pooled = qchk.Problem.of(m)
    theta = pooled.aln()
    for k in range(3):                                                  # three steps, each from the checker's (pooled) theta: one table for all cells
        for tensors in ((False, True) if k == 0 else (k == 1,)):
            ptr, loc, got, info = _qc(m, tensors, theta_in=theta, max_iters=1, tol=0.0)
            for c, cell in enumerate(cs):
                ref, ex = cell.step(theta)
                qchk.agree(cell.scatter(got[ptr[c]:ptr[c + 1]]), ref, cell.tolerance())
                assert info["explained"][c] == ex
        theta = qchk.step(pooled, theta)[0]


# ---- 7. refusals and the empty inputs -----------------------------------------------------------------------------------------------------
FILL = 7.25


def _raw(a, T, H, n_slots, keep=None, scale=None, theta_in=None, max_iters=5, tol=1e-6, null=(), nnz=None, device=False, support=False, capacity=None):
    """ecb_quantify_cells (``support``: ecb_cell_support) -- or, with ``device``, the device entry on CUDA tensors -- on pre-filled outputs ->
    (rc, message, the outputs as numpy, in the order cell_ptr, slot_locus, theta, n_iter, delta, explained, converged)."""
    lib = ecb.load()
    arr = [np.ascontiguousarray(a[k], dtype=np.int32) for k in ("indptrA", "indicesA", "dataA", "indptrN", "indicesN", "dataN")]
    E, nz, S, nzn = len(arr[0]) - 1, len(arr[1]) if nnz is None else nnz, len(arr[3]) - 1, len(arr[4])
    room = n_slots if capacity is None else capacity
    outs = [np.full(S + 1, 77, dtype=np.int64), np.full(room, 77, dtype=np.int32), np.full((room, H), FILL), np.full(S, 77, dtype=np.uint32),
            np.full(S, FILL), np.full(S, 77, dtype=np.int64), np.full(S, 77, dtype=np.uint8)]
    tabs = [None if t is None else np.ascontiguousarray(t, dtype=np.float64) for t in (scale, theta_in)]
    kp = None if keep is None else np.ascontiguousarray(keep, dtype=np.uint8)
    ptr = ecb._ptr
    if device:
        import torch
        dev = lambda x: None if x is None else torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).cuda()      # noqa: E731
        arr, tabs, kp, held = [dev(v) for v in arr], [dev(t) for t in tabs], dev(kp), [dev(o) for o in outs]
        ptr = ecb._dev_ptr
    else:
        held = outs
    p = [None if k in null else ptr(o) for k, o in enumerate(held)]
    head = (0, E, T, H, nz, ptr(arr[0]), ptr(arr[1]), ptr(arr[2]), S, nzn, ptr(arr[3]), ptr(arr[4]), ptr(arr[5]), ptr(kp))
    ns = C.c_uint64(77)
    if support:
        fn = lib.ecb_cell_support_device if device else lib.ecb_cell_support
        rc = fn(*(head + (p[0], p[1], room, C.byref(ns))))
    else:
        fn = lib.ecb_quantify_cells_device if device else lib.ecb_quantify_cells
        rc = fn(*(head + (ptr(tabs[0]), ptr(tabs[1]), max_iters, tol, 0, n_slots) + tuple(p)))
    msg = lib.ecb_last_error(None).decode() if rc else ""
    if device:
        torch.cuda.synchronize()
        outs = [o.cpu().numpy().view(w.dtype) for o, w in zip(held, outs)]
    return rc, msg, outs, ns.value


def _untouched(outs, upto=7):
    return all(bool(np.all(o == (FILL if o.dtype == np.float64 else 77))) for o in outs[:upto])


def test_refusals_leave_the_outputs_untouched_and_the_next_call_works():
    m, theta_in, scale = _edge_matrix(3)
    T, H = m.num_loci, m.num_haplotypes
    good = dict(indptrA=m.indptrA, indicesA=m.indicesA, dataA=m.dataA, indptrN=m.indptrN, indicesN=m.indicesN, dataN=m.dataN)
    nnz, nnz_n, E = len(m.indicesA), len(m.indicesN), m.num_reads
    lens = np.diff(m.indptrA)
    two = int(np.flatnonzero(lens >= 2)[3])
    s0 = int(m.indptrA[two])
    mid_e = int(np.flatnonzero(lens > 0)[200])
    cs = cq.cells(m)
    want_ptr, want_loc = cq.expected_support(cs)
    n_slots = int(want_ptr[-1])
    bad = []

    def case(what, text, **kw):
        for k, (at, v) in list(kw.items()):
            x = np.array(good[k]).copy()
            x[at] = v
            kw[k] = x
        bad.append((what, dict(good, **kw), text))
    # everything ecb_quantify refuses, with its codes
    case("column >= T", "malformed CSR: a locus at or beyond n_loci", indicesA=(nnz // 2, T))
    case("bit >= H", "malformed CSR: a haplotype bit at or beyond n_haplotypes", dataA=(0, 1 << H))
    case("unsorted columns", "malformed CSR: columns not strictly ascending within a row", indicesA=(slice(s0, s0 + 2), [m.indicesA[s0 + 1], m.indicesA[s0]]))
    A_PTR = "malformed CSR: row pointers do not start at 0, go backwards or do not end at nnz"
    case("a falling row pointer", A_PTR, indptrA=(slice(mid_e, mid_e + 2), [m.indptrA[mid_e + 1], m.indptrA[mid_e]]))
    case("indptr[E] below nnz", A_PTR, indptrA=(-1, nnz - 1))
    case("EC index at E", "malformed N: an EC index at or beyond n_ecs", indicesN=(nnz_n // 2, E))
    case("negative count", "malformed N: a negative count", dataN=(nnz_n - 1, -2))
    N_PTR = "malformed N: column pointers do not start at 0, go backwards or do not end at nnz_n"
    case("N's first pointer", N_PTR, indptrN=(0, 1))
    case("a falling column pointer", N_PTR, indptrN=(2, int(m.indptrN[3]) + 1))
    refs = [c.step(theta_in, scale) for c in cs]
    for device in (False, True):
        for what, a, text in bad:
            for kw in (dict(), dict(scale=scale, theta_in=theta_in)):
                rc, msg, outs, _ = _raw(a, T, H, n_slots, device=device, **kw)
                assert rc == -5 and text in msg, (what, device, rc, msg)
                assert _untouched(outs), (what, device)
            rc, msg, outs, ns = _raw(a, T, H, n_slots, device=device, support=True)
            assert rc == -5 and text in msg and _untouched(outs, 2) and ns == 77, (what, device, rc, msg)
        rc, msg, outs, _ = _raw(good, T, H, n_slots, nnz=1 << 30, device=device)
        assert rc == -8 and _untouched(outs), (device, rc, msg)
        for name in ("scale", "theta_in"):
            for v in (np.nan, np.inf, -1e-300):
                for at in ((0, 0), (H - 1, T - 1)):
                    t = np.array(scale if name == "scale" else theta_in)
                    t[at] = v
                    rc, msg, outs, _ = _raw(good, T, H, n_slots, device=device, **{"scale": scale, "theta_in": theta_in, name: t})
                    assert rc == -5 and "an entry of %s is NaN, infinite or negative" % name in msg, (name, v, device, rc, msg)
                    assert _untouched(outs), (name, v, device)
        # a NaN or negative tol, a null cell_ptr, slot_locus or theta
        for kw in (dict(tol=float("nan")), dict(tol=-1e-9), dict(null=(0,)), dict(null=(1,)), dict(null=(2,))):
            rc, msg, outs, _ = _raw(good, T, H, n_slots, device=device, **kw)
            assert rc == -1 and _untouched(outs), (kw, device, rc, msg)
        rc, msg, outs, _ = _raw(good, T, H, n_slots, device=device, support=True, null=(0,))
        assert rc == -1 and _untouched(outs, 2)
        # an n_slots one too small, one too large: the text names both numbers
        for off in (-1, 1):
            rc, msg, outs, _ = _raw(good, T, H, n_slots + off, device=device, theta_in=theta_in, scale=scale)
            assert rc == -1 and str(n_slots + off) in msg and str(n_slots) in msg.replace(str(n_slots + off), "", 1), (off, device, rc, msg)
            assert _untouched(outs), (off, device)
        rc, msg, outs, _ = _raw(good, T, H, 1 << 31, device=device, capacity=1)
        assert rc == -8 and _untouched(outs), (device, rc, msg)
        # a slot_locus too small for the support is left alone; cell_ptr and n_slots are still given
        rc, msg, outs, ns = _raw(good, T, H, n_slots, device=device, support=True, capacity=n_slots - 1)
        assert rc == 0 and ns == n_slots and np.array_equal(outs[0], want_ptr) and _untouched(outs[1:2])
        # the call after the refusals: the device is unharmed; the per-cell outputs may be NULL
        for null in ((), (3, 4, 5, 6)):
            rc, msg, outs, _ = _raw(good, T, H, n_slots, scale=scale, theta_in=theta_in, max_iters=1, tol=0.0, device=device, null=null)
            assert rc == 0, msg
            assert np.array_equal(outs[0], want_ptr) and np.array_equal(outs[1], want_loc)
            for c, (cell, (ref, ex)) in enumerate(zip(cs, refs)):
                qchk.agree(cell.scatter(outs[2][want_ptr[c]:want_ptr[c + 1]]), ref, cell.tolerance())
                assert null or (outs[5][c] == ex and outs[3][c] == (0 if cell.empty() else 1))
            assert not null or _untouched(outs[3:])


def test_the_empty_inputs_succeed():
    T, H = 5, 3
    for a, S in ((dict(indptrA=[0], indicesA=[], dataA=[], indptrN=[0, 0, 0], indicesN=[], dataN=[]), 2),                     # E = 0
                 (dict(indptrA=[0, 0, 0, 0], indicesA=[], dataA=[], indptrN=[0, 2, 2], indicesN=[0, 2], dataN=[4, 1]), 2),       # nnz = 0
                 (dict(indptrA=[0, 1, 3], indicesA=[0, 1, 4], dataA=[1, 7, 2], indptrN=[0], indicesN=[], dataN=[]), 0)):         # S = 0
        for kw in (dict(), dict(theta_in=np.ones((H, T)), scale=np.ones((H, T)))):
            for device in (False, True):
                rc, msg, outs, _ = _raw(a, T, H, 0, device=device, **kw)
                assert rc == 0, msg
                assert not outs[0].any() and all(not o[:S].any() for o in outs[3:6]) and outs[6].all()
                rc, msg, outs, ns = _raw(a, T, H, 0, device=device, support=True)
                assert rc == 0 and ns == 0 and not outs[0].any(), msg
            bad = dict(kw, scale=np.full((H, T), np.nan))               # an empty input is validated like any other
            rc, msg, outs, _ = _raw(a, T, H, 0, device=True, **bad)
            assert rc == -5 and _untouched(outs), (rc, msg)
            rc, msg, outs, _ = _raw(a, T, H, 1, device=True, **kw)
            assert rc == -1 and _untouched(outs), (rc, msg)


# ---- 9. the command -----------------------------------------------------------------------------------------------------------------------
def test_the_command_writes_what_quantify_cells_returns_and_reads_back_exactly(tmp_path):
    m, cs = ms()
    out, rep = str(tmp_path / "o.tsv"), str(tmp_path / "r.tsv")
    env = dict(os.environ)
    env.pop("ALNTOOLS_GPUS", None)
    env["ALNTOOLS_TORCH"] = "0"
    two = [m.sname[3], m.sname[190]]
    for extra, keep in ((["-s", two[0], "-s", two[1], "-i", "40", "-t", "1e-5"], np.isin(np.arange(m.num_samples), [3, 190])), (["-i", "40", "-t", "1e-5"], None)):
        r = subprocess.run([sys.executable, "-m", "alntools_amd.cli", "ecquant-cells", MS, out, "--report", rep, "-v"] + extra, cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        ptr, loc, theta, info = _qc(m, cell_keep=keep, max_iters=40, tol=1e-5)
        lines = [ln.split("\t") for ln in open(out).read().splitlines()]
        assert lines[0] == ["sample", "locus"] + m.hname + ["total"] and len(lines) == 1 + len(loc)
        cell_of = np.repeat(np.arange(m.num_samples), np.diff(ptr))
        assert [ln[0] for ln in lines[1:]] == [m.sname[c] for c in cell_of] and [ln[1] for ln in lines[1:]] == [m.lname[t] for t in loc]
        back = np.array([[float(v) for v in ln[2:]] for ln in lines[1:]])
        assert back[:, :-1].tobytes() == theta.tobytes() and np.array_equal(back[:, -1], theta.sum(axis=1))
        assert open(rep).read() == bin_utils.cells_report(m.sname, info, keep)
        assert len(open(rep).read().splitlines()) == 1 + (m.num_samples if keep is None else 2)
        os.remove(out)
        os.remove(rep)
    r = subprocess.run([sys.executable, "-m", "alntools_amd.cli", "ecquant-cells", MS, out, "--report", rep, "-s", "CELL_NOPE"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "Error: sample CELL_NOPE is not in" in r.stderr and not os.path.exists(out) and not os.path.exists(rep)
