"""ecquant's hierarchical models per cell on the GPU (``ecb_quantify_cells_model*``) against the step pairs recorded from the reference's own
factors and against the cell model checker (``tests/cell_model_checker.py``): every recorded (cell, model, k) through both entry points, one
rule for every route (both entries, every batching, a cell alone, the scratch poisoned), the merged ``ecb.quantify_model(sample=c)`` on the
masked table, model 4 against ``ecb.quantify_cells`` byte for byte, the support rule, every cell's own stop, the paths' edges, the deviation's
rows, every refusal with its outputs untouched, the empty inputs and the command.

The tolerance of one step of one cell is derived in ``test_ecquant_cell_models.py``: ``CellGrouping.tolerance(model)`` with the cell's own B,
L, M and R, relative, entry by entry, the same entries 0."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from alntools_amd import bin_utils, ecb

import cell_model_checker as cm
import cell_quant_checker as cq
import quant_checker as qchk
import quant_model_checker as mchk
from test_ecquant_cell_models import GRP, MS, QC_LONG_COL, QC_LONG_ROW, Q_LONG_GENE, TPB, per_x_bytes
from test_gpu_ecquant_cells import EDGE_CELLS, EDGE_H, INFO, _args, _blob, _cell_blob, _edge_matrix, _mat, _np
from test_quant_constants import Q_BATCH

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MODELS = (1, 2, 3)
_kept = {}


def _qcm(m, gene, G, model, tensors=False, cell_keep=None, scale=None, theta_in=None, **kw):
    """ecb.quantify_cells_model over an ECMatrices -> (cell_ptr, slot_locus, theta, info) as numpy, through the host entry or, with CUDA
    tensors, the device entry."""
    if tensors:
        import torch
        scale, theta_in = (None if t is None else torch.as_tensor(np.asarray(t, dtype=np.float64), device="cuda") for t in (scale, theta_in))
        gene = torch.as_tensor(np.asarray(gene, dtype=np.int32), device="cuda")
    ptr, loc, theta, info = ecb.quantify_cells_model(*_args(m, tensors), gene=gene, n_genes=G, model=model, cell_keep=cell_keep, scale=scale,
                                                     theta_in=theta_in, **kw)
    if tensors:
        assert ptr.is_cuda and loc.is_cuda and theta.is_cuda and all(info[k].is_cuda for k in INFO)
    ptr, loc, theta = _np(ptr), _np(loc), _np(theta)
    info = {k: _np(info[k]) for k in INFO}
    S = m.num_samples
    assert ptr.shape == (S + 1,) and ptr.dtype == np.int64 and loc.dtype == np.int32 and theta.dtype == np.float64
    assert theta.shape == (len(loc), m.num_haplotypes) and ptr[0] == 0 and ptr[-1] == len(loc) and all(info[k].shape == (S,) for k in INFO)
    return ptr, loc, theta, info


def _at(res, q, c):
    """Cell c's theta of a result, dense H x T."""
    return q.cell.scatter(res[2][res[0][c]:res[0][c + 1]])


# ---- 1. the recorded pairs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,model,k", cm.TRIPLES, ids=cm.TRIPLE_IDS)
def test_every_recorded_triple_through_both_entry_points(case, model, k):
    m, cs, gene, G, qs, z = cm.ms()
    c = case["cell"]
    q = qs[c]
    theta_k, ref = cm.pair(z, case, model, k)
    for tensors in (False, True):
        res = _qcm(m, gene, G, model, tensors, theta_in=theta_k, max_iters=1, tol=0.0)       # all 338 cells from this cell's theta_k
        got = _at(res, q, c)
        worst = qchk.agree(got, ref, q.tolerance(model))
        print("cell %d model %d k=%d %s: worst relative difference %.3g, bound %.3g" % (c, model, k, "device" if tensors else "host", worst, q.tolerance(model)))
        assert np.array_equal(res[1][res[0][c]:res[0][c + 1]], q.cell.support) and res[3]["n_iter"][c] == 1 and res[3]["explained"][c] == q.cell.W
        assert abs(float(got.sum()) - q.cell.W) <= q.tolerance(model) * q.cell.W


# ---- 2. one rule for every route ----------------------------------------------------------------------------------------------------------
def _routes(model):
    """The full run by every route; -> the bytes all of them gave."""
    m, cs, gene, G, qs, z = cm.ms()
    kw = dict(max_iters=2 * Q_BATCH + 3, tol=1e-4)                      # (some cells stop early, some run out of steps)
    first = _qcm(m, gene, G, model, **kw)
    blob = _blob(first)
    assert 0 < first[3]["converged"].sum() < m.num_samples
    x = np.array([c.row_len.sum() for c in cs])
    per_x = per_x_bytes(m.num_haplotypes, model)
    for tensors, more in ((True, {}), (False, dict(budget_bytes=1)), (True, dict(budget_bytes=1)),
                          (False, dict(budget_bytes=int(x.sum() // 5 + 1) * per_x)), (True, dict(budget_bytes=int(x.sum() // 3) * per_x)),
                          (True, dict(budget_bytes=0))):
        assert _blob(_qcm(m, gene, G, model, tensors, **dict(kw, **more))) == blob, (tensors, more)
    assert x.max() < x.sum() // 5                                       # (those budgets cut a handful of batches, none of one cell)
    for c in (0, m.num_samples - 1, int(np.argmax(x))):                 # first, last, largest
        keep = np.zeros(m.num_samples, dtype=np.uint8)
        keep[c] = 1
        for tensors in (False, True):
            alone = _qcm(m, gene, G, model, tensors, cell_keep=keep, **kw)
            assert _cell_blob(alone, c) == _cell_blob(first, c) and alone[0][-1] == len(cs[c].support)
            assert alone[3]["converged"][np.arange(m.num_samples) != c].all() and not alone[3]["n_iter"][np.arange(m.num_samples) != c].any()
    return blob


@pytest.mark.parametrize("model", MODELS)
def test_one_rule_for_every_route(model):
    _kept["routes%d" % model] = _routes(model)


def _digest():
    h = hashlib.sha256()
    for key, make in [("routes%d" % model, lambda model=model: _routes(model)) for model in MODELS] + [("edge2", lambda: _edge_case(2))]:
        if key not in _kept:
            _kept[key] = make()
        h.update(_kept[key])
    return h.hexdigest()


def test_everything_once_more_with_the_scratch_poisoned_gives_the_same_bits():
    """One child process with ECB_POISON_SCRATCH=1 repeats the routes of every model and an edge case: every buffer the library allocates is
    filled with 0x01 first, so a pass that relied on fresh memory being 0 gives other bits than this process."""
    env = dict(os.environ)
    env["ECB_POISON_SCRATCH"] = "1"
    env["ALNTOOLS_TORCH"] = "1"
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_ecquant_cell_models as t; print('digest', t._digest())" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "digest " + _digest() in r.stdout


# ---- 3. the merged code on the masked table, 4. model 4, 5. the support rule -----------------------------------------------------------------
def _positive_table(m):
    rng = np.random.default_rng(5)
    return rng.random((m.num_haplotypes, m.num_loci)) * 10 + 0.01


@pytest.mark.parametrize("model", MODELS)
def test_a_cell_is_quantify_model_of_its_sample_on_the_masked_table(model):
    m, cs, gene, G, qs, z = cm.ms()
    theta_in = _positive_table(m)
    x = np.array([c.row_len.sum() for c in cs])
    one = _qcm(m, gene, G, model, theta_in=theta_in, max_iters=1, tol=0.0)
    a = (m.indptrA, m.indicesA, m.dataA, m.num_loci, m.num_haplotypes, m.indptrN, m.indicesN, m.dataN)
    for c in sorted({0, m.num_samples - 1, int(np.argmax(x))} | {case["cell"] for case in cm.CASES}):
        q = qs[c]
        ref, rinfo = ecb.quantify_model(*a, gene=gene, n_genes=G, model=model, sample=c, theta_in=q.masked(theta_in), max_iters=1, tol=0.0)
        qchk.agree(_at(one, q, c), ref, q.tolerance(model))            # (the bound is that of two computed results)
        assert rinfo["explained"] == one[3]["explained"][c] == q.cell.W
    # theta_in NULL: the two start from the same theta_0, aln being 0 outside the support
    run = _qcm(m, gene, G, model, max_iters=1, tol=0.0)
    for c in (0, 3):
        ref, rinfo = ecb.quantify_model(*a, gene=gene, n_genes=G, model=model, sample=c, max_iters=1, tol=0.0)
        qchk.agree(_at(run, qs[c], c), ref, qs[c].tolerance(model))
        assert rinfo["explained"] == run[3]["explained"][c] and run[3]["n_iter"][c] == 1


def test_model_4_returns_the_bytes_of_quantify_cells():
    m, cs, gene, G, qs, z = cm.ms()
    theta_in = _positive_table(m)
    scale = 1.0 / np.asarray(m.lengths).T
    for kw in (dict(max_iters=2 * Q_BATCH + 3, tol=1e-4), dict(theta_in=theta_in, scale=scale, max_iters=2, tol=0.0), dict(max_iters=0)):
        for tensors in (False, True):
            t = {k: v for k, v in kw.items()}
            if tensors:
                import torch
                t.update({k: torch.as_tensor(v, device="cuda") for k, v in kw.items() if k in ("theta_in", "scale")})
            flat = ecb.quantify_cells(*_args(m, tensors), **t)
            flat = (_np(flat[0]), _np(flat[1]), _np(flat[2]), {k: _np(flat[3][k]) for k in INFO})
            assert _blob(_qcm(m, gene, G, 4, tensors, **kw)) == _blob(flat), (kw.keys(), tensors)


@pytest.mark.parametrize("model", MODELS)
def test_phi_runs_over_the_cells_support_only(model):
    m, cs, gene, G, qs, z = cm.ms()
    theta_in = _positive_table(m)
    assert (theta_in > 0).all()
    # on the CPU first: a gene partly inside a cell's support, and the unmasked table gives another answer than the masked one
    partly = [c for c, q in enumerate(qs) if not q.cell.empty() and len(q.cell.rows) > 5
              and any((gene == g).sum() > (gene[q.cell.support] == g).sum() for g in np.unique(gene[q.cell.support]))][:4]
    assert len(partly) == 4
    want = {}
    for c in partly:
        q = qs[c]
        masked, ex = q.step(model, q.masked(theta_in))
        unmasked, _ = mchk.step(q, model, theta_in)
        on = masked > 0
        assert (np.abs(unmasked - masked)[on] / masked[on]).max() > 100 * q.tolerance(model), c
        want[c] = (masked, ex)
    for tensors in (False, True):
        res = _qcm(m, gene, G, model, tensors, theta_in=theta_in, max_iters=1, tol=0.0)
        for c, (masked, ex) in want.items():
            qchk.agree(_at(res, qs[c], c), masked, qs[c].tolerance(model))
            assert res[3]["explained"][c] == ex


# ---- 6. independent stops -----------------------------------------------------------------------------------------------------------------
TOL, ITERS = 1e-6, 300
#: per model, of the checker's runs: the distinct stops, the cells that stop after one step, those that run out of steps, those beyond 2 Q_BATCH
SPREAD = {1: (95, 78, 12, 245), 2: (98, 78, 12, 242), 3: (101, 78, 14, 243)}


@pytest.mark.parametrize("model", MODELS)
def test_every_cell_stops_at_its_own_step(model):
    m, cs, gene, G, qs, z = cm.ms()
    runs = [q.run(model, max_iters=ITERS, tol=TOL) for q in qs]
    n = np.array([i["n_iter"] for _, i in runs])
    conv = np.array([i["converged"] for _, i in runs])
    # the spread the checker computes, asserted before the device is looked at
    assert (len(set(n.tolist())), int((n == 1).sum()), int((~conv).sum()), int((n > 2 * Q_BATCH).sum())) == SPREAD[model]
    res = {}
    for tensors in (False, True):
        res[tensors] = ptr, loc, theta, info = _qcm(m, gene, G, model, tensors, max_iters=ITERS, tol=TOL)
        for c, (q, (_, ri)) in enumerate(zip(qs, runs)):
            k = int(info["n_iter"][c])
            at = ri if k == ri["n_iter"] else q.run(model, max_iters=k, tol=0.0)[1]        # (the checker's figures at the device's step)
            bound = q.tolerance(model) * max(k, 1)
            assert abs(k - ri["n_iter"]) <= 1, (c, k, ri["n_iter"])
            if bool(info["converged"][c]) != ri["converged"]:           # only within one step of the stop: the last step allowed, or the one after it
                assert ri["n_iter"] >= ITERS - 1 if ri["converged"] else q.run(model, max_iters=ITERS + 1, tol=TOL)[1]["converged"], c
            if info["converged"][c]:
                assert info["delta"][c] <= TOL * q.cell.W
            else:
                assert k == ITERS, (c, k)
            assert abs(info["delta"][c] - at["delta"]) <= bound * at["explained"], c
            assert abs(int(info["explained"][c]) - at["explained"]) <= bound * at["explained"], c
    assert _blob(res[False]) == _blob(res[True])


# ---- 7. the paths' edges ------------------------------------------------------------------------------------------------------------------
N_RANDOM_GENES = 150


def _edge_genes(m, cs, H, seed=77):
    """A seeded gene map over the edge matrix's 700 loci whose ids interleave in locus order: random genes, then -- drawn from the support of
    the cell ``long_rows`` -- three genes of Q_LONG_GENE - 1, Q_LONG_GENE and Q_LONG_GENE + 1 members, five singletons, and the loci of the
    single row of the cell ``one_entry`` as one gene."""
    rng = np.random.default_rng(seed + H)
    by = dict(zip(EDGE_CELLS, cs))
    gene = rng.integers(0, N_RANDOM_GENES, size=m.num_loci).astype(np.int32)
    e = int(m.indicesN[m.indptrN[EDGE_CELLS.index("one_entry")]])
    one_row = m.indicesA[m.indptrA[e]:m.indptrA[e + 1]]
    free = np.setdiff1d(by["long_rows"].support, one_row)
    pick = rng.permutation(free)
    at, G = 0, N_RANDOM_GENES
    for n in (Q_LONG_GENE - 1, Q_LONG_GENE, Q_LONG_GENE + 1) + (1,) * 5:
        gene[pick[at:at + n]] = G
        at, G = at + n, G + 1
    gene[one_row] = G
    return gene, G + 1


def _edge_setup(H):
    """(the edge matrix, theta_in, scale, its cells, gene, G, one CellGrouping per cell), each shape asserted before it is used."""
    m, theta_in, scale = _edge_matrix(H)
    cs = cq.cells(m)
    gene, G = _edge_genes(m, cs, H)
    qs = cm.groupings(cs, gene, G)
    by = dict(zip(EDGE_CELLS, qs))
    # the matrix and the gene map really hold what they were built for
    lr = by["long_rows"]
    members = np.bincount(gene[lr.cell.support], minlength=G)
    assert members[N_RANDOM_GENES:N_RANDOM_GENES + 3].tolist() == [Q_LONG_GENE - 1, Q_LONG_GENE, Q_LONG_GENE + 1] and lr.M == Q_LONG_GENE + 1
    for g in range(N_RANDOM_GENES, N_RANDOM_GENES + 3):                 # the members are scattered: other genes' slots lie between them
        at = np.flatnonzero(gene[lr.cell.support] == g)
        assert at[-1] - at[0] + 1 > 2 * len(at)
    assert np.bincount(gene, minlength=G)[N_RANDOM_GENES + 3:N_RANDOM_GENES + 8].tolist() == [1] * 5 and members[N_RANDOM_GENES + 3:N_RANDOM_GENES + 8].tolist() == [1] * 5
    assert by["one_entry"].R == 1 and len(by["one_entry"].cell.rows) == 1 and len(by["one_entry"].cell.support) > 1
    assert lr.R > 100 and lr.cell.row_len.tolist()[:3] == [QC_LONG_ROW - 1, QC_LONG_ROW, QC_LONG_ROW + 1]          # rows touching many genes
    assert by["long_cols"].cell.col_len[:3].tolist() == [QC_LONG_COL - 1, QC_LONG_COL, QC_LONG_COL + 1]
    both = np.intersect1d(gene[by["random"].cell.support], gene[by["random2"].cell.support])
    assert len(both) > 20                                               # the same genes in two cells of one batch
    items = [len(by[c].cell.support) * H for c in ("chunk_lo", "chunk_at", "chunk_hi")]
    assert items == [(TPB // H - 1) * H, TPB // H * H, (TPB // H + 1) * H]
    assert len(by["twice"].cell.rows) == 3 and (m.dataA == 0).any() and (m.dataN == 0).any()
    assert all(by[c].cell.empty() for c in ("empty_first", "empty_middle", "empty_last", "zero_counts", "zero_masks")) and cs[0].empty() and cs[-1].empty()
    return m, theta_in, scale, cs, gene, G, qs


def _edge_case(H):
    m, theta_in, scale, cs, gene, G, qs = _edge_setup(H)
    want_ptr, want_loc = cq.expected_support(cs)
    out = b""
    for sc in (None, scale):
        for model in MODELS:
            steps = [q.step(model, theta_in, sc) for q in qs]
            assert sum(ex < q.cell.W for q, (_, ex) in zip(qs, steps)) >= 2      # rows with a count whose targets all have theta = 0
            steps0 = [q.step(model, q.p.aln(), sc) for q in qs]
            for tensors in (False, True):
                for refs, res in ((steps, _qcm(m, gene, G, model, tensors, scale=sc, theta_in=theta_in, max_iters=1, tol=0.0)),
                                  (steps0, _qcm(m, gene, G, model, tensors, scale=sc, max_iters=1, tol=0.0))):
                    ptr, loc, theta, info = res
                    assert np.array_equal(ptr, want_ptr) and np.array_equal(loc, want_loc)
                    for c, (q, (ref, ex)) in enumerate(zip(qs, refs)):
                        qchk.agree(_at(res, q, c), ref, q.tolerance(model))
                        assert info["explained"][c] == ex and info["n_iter"][c] == (0 if q.cell.empty() else 1), (EDGE_CELLS[c], model, tensors)
                        assert not q.cell.empty() or (info["converged"][c] and info["delta"][c] == 0)
                    if refs is steps0:
                        assert all(info["explained"][c] == q.cell.W for c, q in enumerate(qs))
                    out += _blob(res)
    return out


@pytest.mark.parametrize("H", EDGE_H)
def test_edges(H):
    _kept["edge%d" % H] = _edge_case(H)


# ---- 8. the deviation's rows --------------------------------------------------------------------------------------------------------------
def test_the_deviation_cases_stacked_as_three_cells_lose_no_mass():
    """Each hand-built matrix as a cell of its own over its own three loci (one shared theta table has room for the three thetas)."""
    dev = cm.deviation_cells()
    rows = [(np.asarray(csr[1][csr[0][r]:csr[0][r + 1]]) + 3 * k, np.asarray(csr[2][csr[0][r]:csr[0][r + 1]])) for k, d in enumerate(dev) for csr in [d[2]]
            for r in range(3)]
    indptr = np.cumsum([0] + [len(r[0]) for r in rows])
    m = _mat(2, 9, indptr, np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows]), [0, 3, 6, 9], np.arange(9), [10, 3, 5] * 3)
    gene, G = np.concatenate([np.asarray(d[4]) + 2 * k for k, d in enumerate(dev)]).astype(np.int32), 6
    theta_in = np.concatenate([d[6] for d in dev], axis=1)
    qs = cm.groupings(cq.cells(m), gene, G)
    for k, d in enumerate(dev):                                         # each cell is the hand-built problem, moved by 3 k loci
        assert np.array_equal(qs[k].p.bit_row, d[3].p.bit_row) and np.array_equal(qs[k].p.bit_flat % 9, d[3].p.bit_flat % 3 + 3 * k) and qs[k].cell.W == 18
    for model in MODELS:
        for tensors in (False, True):
            res = _qcm(m, gene, G, model, tensors, theta_in=theta_in, max_iters=1, tol=0.0)
            for c, q in enumerate(qs):
                ref, ex = q.step(model, theta_in)
                got = _at(res, q, c)
                qchk.agree(got, ref, q.tolerance(model))
                assert ex == 18 == res[3]["explained"][c] and abs(float(got.sum()) - 18.0) <= q.tolerance(model) * 18.0          # no mass is lost
                assert not got[theta_in == 0].any()


# ---- 9. refusals, 10. the empty inputs ----------------------------------------------------------------------------------------------------
FILL = 7.25


def _raw(a, T, H, n_slots, gene, G, model, keep=None, scale=None, theta_in=None, max_iters=5, tol=1e-6, null=(), nnz=None, device=False, no_gene=False):
    """ecb_quantify_cells_model -- or, with ``device``, the device entry on CUDA tensors -- on pre-filled outputs -> (rc, message, the outputs
    as numpy, in the order cell_ptr, slot_locus, theta, n_iter, delta, explained, converged)."""
    lib = ecb.load()
    arr = [np.ascontiguousarray(a[k], dtype=np.int32) for k in ("indptrA", "indicesA", "dataA", "indptrN", "indicesN", "dataN")]
    E, nz, S, nzn = len(arr[0]) - 1, len(arr[1]) if nnz is None else nnz, len(arr[3]) - 1, len(arr[4])
    outs = [np.full(S + 1, 77, dtype=np.int64), np.full(n_slots, 77, dtype=np.int32), np.full((n_slots, H), FILL), np.full(S, 77, dtype=np.uint32),
            np.full(S, FILL), np.full(S, 77, dtype=np.int64), np.full(S, 77, dtype=np.uint8)]
    tabs = [None if t is None else np.ascontiguousarray(t, dtype=np.float64) for t in (scale, theta_in)]
    kp = None if keep is None else np.ascontiguousarray(keep, dtype=np.uint8)
    gn = np.ascontiguousarray(gene, dtype=np.int32)
    ptr = ecb._ptr
    if device:
        import torch
        dev = lambda x: None if x is None else torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).cuda()      # noqa: E731
        arr, tabs, kp, gn, held = [dev(v) for v in arr], [dev(t) for t in tabs], dev(kp), dev(gn), [dev(o) for o in outs]
        ptr = ecb._dev_ptr
    else:
        held = outs
    p = [None if k in null else ptr(o) for k, o in enumerate(held)]
    fn = lib.ecb_quantify_cells_model_device if device else lib.ecb_quantify_cells_model
    rc = fn(0, E, T, H, nz, ptr(arr[0]), ptr(arr[1]), ptr(arr[2]), S, nzn, ptr(arr[3]), ptr(arr[4]), ptr(arr[5]), ptr(kp), ptr(tabs[0]), ptr(tabs[1]),
            max_iters, tol, 0, G, None if no_gene else ptr(gn), model, n_slots, *p)
    msg = lib.ecb_last_error(None).decode() if rc else ""
    if device:
        torch.cuda.synchronize()
        outs = [o.cpu().numpy().view(w.dtype) for o, w in zip(held, outs)]
    return rc, msg, outs


def _untouched(outs):
    return all(bool(np.all(o == (FILL if o.dtype == np.float64 else 77))) for o in outs)


def test_refusals_leave_the_outputs_untouched_and_the_next_call_works():
    m, theta_in, scale = _edge_matrix(3)
    T, H = m.num_loci, m.num_haplotypes
    good = dict(indptrA=m.indptrA, indicesA=m.indicesA, dataA=m.dataA, indptrN=m.indptrN, indicesN=m.indicesN, dataN=m.dataN)
    cs = cq.cells(m)
    gene, G = _edge_genes(m, cs, 3)
    qs = cm.groupings(cs, gene, G)
    want_ptr, want_loc = cq.expected_support(cs)
    n_slots = int(want_ptr[-1])
    nnz, nnz_n = len(m.indicesA), len(m.indicesN)

    def changed(k, at, v):
        x = np.array(good[k]).copy()
        x[at] = v
        return dict(good, **{k: x})
    for device in (False, True):
        for model in (1, 2, 3, 4):
            # a gene id out of range, at either end, for every model
            for at, v in ((0, G), (T - 1, -1), (T // 2, 1 << 30)):
                bad = gene.copy()
                bad[at] = v
                rc, msg, outs = _raw(good, T, H, n_slots, bad, G, model, device=device, scale=scale, theta_in=theta_in)
                assert rc == -5 and "a gene id outside [0, n_genes)" in msg and _untouched(outs), (device, model, at, rc, msg)
            # a null gene, no gene at all
            rc, msg, outs = _raw(good, T, H, n_slots, gene, G, model, device=device, no_gene=True)
            assert rc == -1 and _untouched(outs), (device, model, rc, msg)
            rc, msg, outs = _raw(good, T, H, n_slots, gene, 0, model, device=device)
            assert rc == -1 and _untouched(outs), (device, model, rc, msg)
            # a wrong n_slots: the text names both numbers
            for off in (-1, 1):
                rc, msg, outs = _raw(good, T, H, n_slots + off, gene, G, model, device=device, theta_in=theta_in, scale=scale)
                assert rc == -1 and str(n_slots + off) in msg and str(n_slots) in msg.replace(str(n_slots + off), "", 1), (off, device, model, rc, msg)
                assert _untouched(outs), (off, device, model)
        for model in (0, 5, 1 << 31):
            rc, msg, outs = _raw(good, T, H, n_slots, gene, G, model, device=device)
            assert rc == -1 and "no such model" in msg and _untouched(outs), (device, model, rc, msg)
        # the inherited refusals, with their codes
        for model in (1, 2, 3):
            for what, a, text in (("column >= T", changed("indicesA", nnz // 2, T), "malformed CSR: a locus at or beyond n_loci"),
                                  ("bit >= H", changed("dataA", 0, 1 << H), "malformed CSR: a haplotype bit at or beyond n_haplotypes"),
                                  ("negative count", changed("dataN", nnz_n - 1, -2), "malformed N: a negative count"),
                                  ("N's first pointer", changed("indptrN", 0, 1), "malformed N: column pointers do not start at 0")):
                rc, msg, outs = _raw(a, T, H, n_slots, gene, G, model, device=device, scale=scale, theta_in=theta_in)
                assert rc == -5 and text in msg and _untouched(outs), (what, device, model, rc, msg)
            rc, msg, outs = _raw(good, T, H, n_slots, gene, G, model, nnz=1 << 30, device=device)
            assert rc == -8 and _untouched(outs), (device, rc, msg)
            for name in ("scale", "theta_in"):
                t = np.array(scale if name == "scale" else theta_in)
                t[H - 1, T - 1] = np.nan
                rc, msg, outs = _raw(good, T, H, n_slots, gene, G, model, device=device, **{"scale": scale, "theta_in": theta_in, name: t})
                assert rc == -5 and "an entry of %s is NaN, infinite or negative" % name in msg and _untouched(outs), (name, device, rc, msg)
            for kw in (dict(tol=float("nan")), dict(tol=-1e-9), dict(null=(0,)), dict(null=(1,)), dict(null=(2,))):
                rc, msg, outs = _raw(good, T, H, n_slots, gene, G, model, device=device, **kw)
                assert rc == -1 and _untouched(outs), (kw, device, rc, msg)
            # the call after the refusals: the device is unharmed; the per-cell outputs may be NULL
            refs = [q.step(model, theta_in, scale) for q in qs]
            for null in ((), (3, 4, 5, 6)):
                rc, msg, outs = _raw(good, T, H, n_slots, gene, G, model, scale=scale, theta_in=theta_in, max_iters=1, tol=0.0, device=device, null=null)
                assert rc == 0, msg
                assert np.array_equal(outs[0], want_ptr) and np.array_equal(outs[1], want_loc)
                for c, (q, (ref, ex)) in enumerate(zip(qs, refs)):
                    qchk.agree(q.cell.scatter(outs[2][want_ptr[c]:want_ptr[c + 1]]), ref, q.tolerance(model))
                    assert null or (outs[5][c] == ex and outs[3][c] == (0 if q.cell.empty() else 1))
                assert not null or _untouched(outs[3:])


def test_the_empty_inputs_succeed():
    T, H = 5, 3
    gene, G = np.array([0, 1, 1, 2, 0]), 3
    for a, S in ((dict(indptrA=[0], indicesA=[], dataA=[], indptrN=[0, 0, 0], indicesN=[], dataN=[]), 2),                     # E = 0
                 (dict(indptrA=[0, 0, 0, 0], indicesA=[], dataA=[], indptrN=[0, 2, 2], indicesN=[0, 2], dataN=[4, 1]), 2),       # nnz = 0
                 (dict(indptrA=[0, 1, 3], indicesA=[0, 1, 4], dataA=[1, 7, 2], indptrN=[0], indicesN=[], dataN=[]), 0)):         # S = 0
        for model in (1, 2, 3, 4):
            for kw in (dict(), dict(theta_in=np.ones((H, T)), scale=np.ones((H, T)))):
                for device in (False, True):
                    rc, msg, outs = _raw(a, T, H, 0, gene, G, model, device=device, **kw)
                    assert rc == 0, msg
                    assert not outs[0].any() and all(not o[:S].any() for o in outs[3:6]) and outs[6].all()
                # an empty input is validated like any other
                rc, msg, outs = _raw(a, T, H, 0, np.array([0, 1, 3, 2, 0]), G, model, device=True, **kw)
                assert rc == -5 and _untouched(outs), (rc, msg)
                rc, msg, outs = _raw(a, T, H, 1, gene, G, model, device=True, **kw)
                assert rc == -1 and _untouched(outs), (rc, msg)


# ---- 11. the command ----------------------------------------------------------------------------------------------------------------------
def test_the_command_with_a_model_writes_what_quantify_cells_model_returns_and_reads_back_exactly(tmp_path):
    m, cs, gene, G, qs, z = cm.ms()
    out, rep = str(tmp_path / "o.tsv"), str(tmp_path / "r.tsv")
    env = dict(os.environ)
    env.pop("ALNTOOLS_GPUS", None)
    env["ALNTOOLS_TORCH"] = "0"
    two = [m.sname[3], m.sname[190]]
    for extra, keep in ((["-s", two[0], "-s", two[1], "-i", "40", "-t", "1e-5"], np.isin(np.arange(m.num_samples), [3, 190])), (["-i", "40", "-t", "1e-5"], None)):
        r = subprocess.run([sys.executable, "-m", "alntools_amd.cli", "ecquant-cells", MS, out, "--report", rep, "-v", "-M", "2", "-g", GRP] + extra,
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        ptr, loc, theta, info = _qcm(m, gene, G, 2, cell_keep=keep, max_iters=40, tol=1e-5)
        lines = [ln.split("\t") for ln in open(out).read().splitlines()]
        assert lines[0] == ["sample", "locus"] + m.hname + ["total"] and len(lines) == 1 + len(loc)
        cell_of = np.repeat(np.arange(m.num_samples), np.diff(ptr))
        assert [ln[0] for ln in lines[1:]] == [m.sname[c] for c in cell_of] and [ln[1] for ln in lines[1:]] == [m.lname[t] for t in loc]
        back = np.array([[float(v) for v in ln[2:]] for ln in lines[1:]])
        assert back[:, :-1].tobytes() == theta.tobytes() and np.array_equal(back[:, -1], theta.sum(axis=1))
        assert open(rep).read() == bin_utils.cells_report(m.sname, info, keep)
        flat = ecb.quantify_cells(*_args(m, False), cell_keep=keep, max_iters=40, tol=1e-5)
        assert flat[2].tobytes() != theta.tobytes()                    # (the model's answer, not the flat step's)
        os.remove(out)
        os.remove(rep)
    r = subprocess.run([sys.executable, "-m", "alntools_amd.cli", "ecquant-cells", MS, out, "-M", "2"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 1 and "Error: model 2 needs a group file" in r.stderr and not os.path.exists(out)
