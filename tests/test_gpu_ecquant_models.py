"""ecquant's hierarchical models on the GPU (``ecb_quantify_model`` / ``ecb_quantify_model_device``) against the step pairs recorded from
the reference's own factors and against the model checker (``tests/quant_model_checker.py``): every recorded pair through both entry
points, model 4 against ``ecb.quantify`` byte for byte, determinism bit for bit (two calls, host against device entry, a run against
fed-back single steps, all of it once more with the scratch poisoned), the stop, synthetic matrices on both sides of the long-row,
long-column and long-gene thresholds, the hand-built rows of the deviation, every refusal with its outputs untouched, and the command.

The tolerance of one step is derived in ``test_ecquant_models.py`` (``Grouping.tolerance``): relative, entry by entry, the same entries 0;
its terms are computed from the matrix each test uses."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from alntools_amd import bin_utils, ecb

import quant_checker as qchk
import quant_model_checker as mchk
from test_ecquant_models import Q_LONG_GENE
from test_quant_constants import Q_BATCH, Q_LONG_COL, Q_LONG_ROW

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = mchk.GOLDEN
MODELS = (1, 2, 3)


def _names(n, p):
    return ["%s%d" % (p, i) for i in range(n)]


def _mat(H, T, indptrA, indicesA, dataA, indptrN, indicesN, dataN):
    S = len(indptrN) - 1
    return bin_utils.ECMatrices(_names(H, "h"), _names(T, "t"), np.ones((T, H)), _names(S, "s"), indptrA, indicesA, dataA, indptrN, indicesN, dataN)


def _quant(m, gene, G, model, tensors=False, sample=None, scale=None, theta_in=None, **kw):
    """ecb.quantify_model over an ECMatrices -> (theta as numpy, info), through the host entry or, with CUDA tensors, the device entry."""
    a = [m.indptrA, m.indicesA, m.dataA, m.indptrN, m.indicesN, m.dataN]
    if tensors:
        import torch
        a = [torch.as_tensor(np.asarray(x, dtype=np.int32), device="cuda") for x in a]
        gene = torch.as_tensor(np.asarray(gene, dtype=np.int32), device="cuda")
        scale, theta_in = (None if t is None else torch.as_tensor(np.asarray(t, dtype=np.float64), device="cuda") for t in (scale, theta_in))
    theta, info = ecb.quantify_model(a[0], a[1], a[2], m.num_loci, m.num_haplotypes, a[3], a[4], a[5], gene, G, model, sample=sample, scale=scale,
                                     theta_in=theta_in, **kw)
    if tensors:
        assert theta.is_cuda
        theta = theta.cpu().numpy()
    assert theta.shape == (m.num_haplotypes, m.num_loci) and theta.dtype == np.float64
    return theta, info


# ---- 1. the recorded pairs, model 4 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,model,k", mchk.TRIPLES, ids=mchk.TRIPLE_IDS)
def test_every_recorded_pair_through_both_entry_points(case, model, k):
    m, q, z, scale = mchk.load_case(case)
    theta, ref = mchk.pair(z, model, k)
    _, explained = mchk.step(q, model, theta, scale)
    bound = q.tolerance(model)
    for tensors in (False, True):
        got, info = _quant(m, q.gene, q.G, model, tensors, case["sample"], scale, theta, max_iters=1, tol=0.0)
        worst = qchk.agree(got, ref, bound)
        print("%s model %d k=%d %s: worst relative difference %.3g, bound %.3g" % (case["name"], model, k, "device" if tensors else "host", worst, bound))
        assert info["n_iter"] == 1 and not info["converged"] and info["explained"] == explained
        assert abs(float(got.sum()) - explained) <= bound * explained


def test_model_4_returns_the_bytes_of_quantify():
    case = mchk.CASES[3]
    m, q, z, scale = mchk.load_case(case)
    a = (m.indptrA, m.indicesA, m.dataA, m.num_loci, m.num_haplotypes, m.indptrN, m.indicesN, m.dataN)
    for kw in (dict(max_iters=0), dict(max_iters=Q_BATCH + 3, tol=0.0), dict(tol=1e-4), dict(theta_in=z[2]["theta_5"], max_iters=2, tol=0.0)):
        flat, finfo = ecb.quantify(*a, scale=scale, **kw)
        for tensors in (False, True):
            got, info = _quant(m, q.gene, q.G, 4, tensors, scale=scale, **kw)
            assert got.tobytes() == flat.tobytes() and info == finfo, (kw, tensors)


def test_theta_0_from_a_null_theta_in_is_aln_exactly():
    for case in mchk.CASES[:3]:
        m, q, z, scale = mchk.load_case(case)
        for model in MODELS:
            got, info = _quant(m, q.gene, q.G, model, model == 2, case["sample"], scale, max_iters=0)
            assert np.array_equal(got, z["theta_0"]) and info == {"n_iter": 0, "delta": 0.0, "explained": 0, "converged": False}


# ---- 2. determinism -----------------------------------------------------------------------------------------------------------------------
def _determinism(case, model, K=7):
    """Two calls, host against device entry, a run of K against K fed-back single steps: all bit for bit.  Returns the bytes compared."""
    m, q, z, scale = mchk.load_case(case)
    s, g, G = case["sample"], q.gene, q.G
    a, ia = _quant(m, g, G, model, False, s, scale, max_iters=K, tol=0.0)
    b, ib = _quant(m, g, G, model, False, s, scale, max_iters=K, tol=0.0)
    d, idv = _quant(m, g, G, model, True, s, scale, max_iters=K, tol=0.0)
    assert a.tobytes() == b.tobytes() and ia == ib, "two calls differ"
    assert a.tobytes() == d.tobytes() and ia == idv, "host and device entry differ"
    assert ia["n_iter"] == K and not ia["converged"]
    theta, _ = _quant(m, g, G, model, False, s, scale, max_iters=0)
    for _ in range(K):
        theta, one = _quant(m, g, G, model, False, s, scale, theta, max_iters=1, tol=0.0)
    assert theta.tobytes() == a.tobytes(), "a run of K is not K single steps"
    assert (one["delta"], one["explained"]) == (ia["delta"], ia["explained"])
    # more steps than the host enqueues between two looks at the device, and a stop in the middle of a batch
    K2 = Q_BATCH + 3
    c, ic = _quant(m, g, G, model, False, s, scale, max_iters=K2, tol=0.0)
    e, _ = _quant(m, g, G, model, False, s, scale, a, max_iters=K2 - K, tol=0.0)
    assert c.tobytes() == e.tobytes() and ic["n_iter"] == K2
    return a.tobytes() + c.tobytes() + repr(sorted(ia.items())).encode() + repr(sorted(ic.items())).encode()


DET = [(c, model) for c in mchk.CASES for model in MODELS]
DET_IDS = ["%s-m%d" % (c["name"], model) for c, model in DET]
_bytes_of = {}          # what this process's own determinism and edge tests compared, kept for the comparison with the poisoned child


def _kept(key, make):
    if key not in _bytes_of:
        _bytes_of[key] = make()
    return _bytes_of[key]


@pytest.mark.parametrize("case,model", DET, ids=DET_IDS)
def test_two_calls_both_entries_and_fed_back_steps_agree_bit_for_bit(case, model):
    _bytes_of[(case["name"], model)] = _determinism(case, model)


def _digest():
    """Every recorded case's determinism checks and every synthetic matrix: a digest of all the bytes they compared."""
    h = hashlib.sha256()
    for case, model in DET:
        h.update(_kept((case["name"], model), lambda: _determinism(case, model)))
    for H in EDGE_H:
        h.update(_kept("edge%d" % H, lambda: _edge_case(H)))
    return h.hexdigest()


def test_everything_once_more_with_the_scratch_poisoned_gives_the_same_bits():
    """One child process with ECB_POISON_SCRATCH=1: every buffer the library allocates is filled with 0x01 first, so a pass that relied on
    fresh memory being 0 gives other bits than this process, whose digest of the same calls the child's must equal."""
    env = dict(os.environ)
    env["ECB_POISON_SCRATCH"] = "1"
    env["ALNTOOLS_TORCH"] = "1"                     # (the child holds tensors: libecb and PyTorch share one HIP runtime, whatever this process set)
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_ecquant_models as t; print('digest', t._digest())" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "digest " + _digest() in r.stdout


# ---- 3. the stop --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_the_run_stops_at_the_checkers_step(model):
    case = mchk.CASES[2]
    assert case["name"] == "ms"
    m, q, z, scale = mchk.load_case(case)
    tol = 1e-9
    ref, rinfo = mchk.run(q, model, tol=tol)
    n = rinfo["n_iter"]
    assert rinfo["converged"] and n > Q_BATCH                          # (more than one look at the device before the stop)
    # delta adds up differences of entries that each carry the step's relative bound times the steps taken: it may be off by that much of
    # what theta adds up to (the explained reads).  Where the checker's delta clears the stop by more than that at steps n - 1 and n, the
    # device stops at exactly n
    bound = q.tolerance(model) * n
    before = mchk.run(q, model, max_iters=n - 1, tol=0.0)[1]
    clear = min(before["delta"] - tol * q.p.W, tol * q.p.W - rinfo["delta"]) > bound * rinfo["explained"]
    for tensors in (False, True):
        got, info = _quant(m, q.gene, q.G, model, tensors, tol=tol)
        at = rinfo if info["n_iter"] == n else mchk.run(q, model, max_iters=info["n_iter"], tol=0.0)[1]
        print("model %d: n_iter %d (checker %d, clear of the stop: %s), delta %r (checker %r), explained %d (checker %d)"
              % (model, info["n_iter"], n, clear, info["delta"], at["delta"], info["explained"], at["explained"]))
        assert abs(info["n_iter"] - n) <= 1 and info["converged"] is True
        assert info["n_iter"] == n or not clear
        assert info["delta"] <= tol * q.p.W
        assert abs(info["delta"] - at["delta"]) <= bound * at["explained"]
        assert info["explained"] == at["explained"]
        if info["n_iter"] == n:
            qchk.agree(got, ref, bound)
        short, sinfo = _quant(m, q.gene, q.G, model, tensors, tol=tol, max_iters=n - 2)
        assert sinfo["converged"] is False and sinfo["n_iter"] == n - 2 and sinfo["delta"] > tol * q.p.W


# ---- 4. the paths' edges ------------------------------------------------------------------------------------------------------------------
EDGE_H = [1, 8, 31]
T_EDGE = 700
BIG = 200                           # members of the third large gene


def _edge_matrix(H, seed=23, E_rand=1500):
    """Seeded.  Genes (their ids shuffled, so that gene order is not target order): one of Q_LONG_GENE members (targets 0 ..), one of
    Q_LONG_GENE + 1, one of BIG, then targets up to 500 in genes of 1 to 4 members dealt at random (a gene's members are not neighbours),
    then singletons.  Rows: E_rand random ones over the columns from 2 on, columns 0 and 1 added to the first Q_LONG_COL and Q_LONG_COL + 1
    of them; a row of Q_LONG_ROW and one of Q_LONG_ROW + 1 non-zeros spread over the three large genes; a row that is one single segment
    (with a stored mask of 0 inside it); a row whose every non-zero is its own gene; some stored masks 0, rows without a weight, and
    targets whose theta_in is 0."""
    rng = np.random.default_rng(seed + H)
    T = T_EDGE
    a, b, c = Q_LONG_GENE, 2 * Q_LONG_GENE + 1, 2 * Q_LONG_GENE + 1 + BIG
    gene = np.empty(T, dtype=np.int64)
    gene[:a], gene[a:b], gene[b:c] = 0, 1, 2
    small = np.repeat(np.arange(120), rng.integers(1, 5, size=120))[:500 - c]
    gene[c:500] = 3 + rng.permutation(small)
    gene[500:] = 3 + 120 + np.arange(T - 500)
    _, gene = np.unique(gene, return_inverse=True)                      # (ids without gaps)
    G = int(gene.max()) + 1
    gene = rng.permutation(G)[gene]
    rows = []
    for e in range(E_rand):
        cols = np.sort(rng.choice(np.arange(2, T), size=int(rng.integers(0, 9)), replace=False))
        lead = [col for col, k in ((0, Q_LONG_COL), (1, Q_LONG_COL + 1)) if e < k]
        rows.append(np.concatenate([np.array(lead, dtype=np.int64), cols]))
    for n in (Q_LONG_ROW, Q_LONG_ROW + 1):
        rows.append(np.sort(rng.choice(np.arange(2, c), size=n, replace=False)))
    one_segment = len(rows)
    rows.append(np.sort(rng.choice(np.arange(b, c), size=20, replace=False)))
    rows.append(np.sort(rng.choice(np.arange(500, T), size=30, replace=False)))
    E = len(rows)
    indptr = np.cumsum([0] + [len(r) for r in rows])
    indices = np.concatenate(rows)
    data = rng.integers(1, 1 << H, size=len(indices), dtype=np.int64)
    data[rng.random(len(data)) < 0.03] = 0                              # stored masks of 0
    data[indptr[40]:indptr[41]] = 0                                     # ... a whole row of them
    data[indptr[one_segment]:indptr[one_segment + 1]] = rng.integers(1, 1 << H, size=20)
    data[indptr[one_segment] + 7] = 0                                   # ... and one inside the single segment
    w = rng.integers(1, 50, size=E)
    w[rng.random(E) < 0.1] = 0                                          # zero-weight rows: N does not list them
    w[E_rand:] = [7, 5, 3, 2]                                           # (the special rows weigh something)
    listed = np.flatnonzero(w)
    m = _mat(H, T, indptr, indices, data, [0, len(listed)], listed, w[listed])
    theta_in = rng.random((H, T)) * 10 + 0.01
    for e in (5, E_rand // 2):                                          # rows whose targets all have theta = 0: d = 0
        theta_in[:, indices[indptr[e]:indptr[e + 1]]] = 0.0
    theta_in[:, rng.choice(np.arange(2, T), size=40, replace=False)] = 0.0          # members without abundance: left out of the denominators
    theta_in[rng.random((H, T)) < 0.05] = 0.0
    scale = 1.0 / rng.integers(1, 3000, size=(H, T))
    return m, gene, G, theta_in, scale, one_segment


def _edge_case(H):
    m, gene, G, theta_in, scale, one_segment = _edge_matrix(H)
    q = mchk.Grouping(qchk.Problem.of(m), gene, G)
    p = q.p
    lens = np.diff(m.indptrA)
    assert lens.max() == Q_LONG_ROW + 1 and (lens == Q_LONG_ROW).any()
    for e in np.flatnonzero(lens >= Q_LONG_ROW):
        assert len(set(gene[m.indicesA[m.indptrA[e]:m.indptrA[e + 1]]])) == 3          # spread over 3 genes
    col = np.bincount(m.indicesA, minlength=m.num_loci)
    assert col[:2].tolist() == [Q_LONG_COL, Q_LONG_COL + 1]
    members = np.sort(np.bincount(gene))[::-1]
    assert members[:3].tolist() == [BIG, Q_LONG_GENE + 1, Q_LONG_GENE] and members[3] <= 4
    seg = m.indicesA[m.indptrA[one_segment]:m.indptrA[one_segment + 1]]
    assert len(set(gene[seg])) == 1 and (m.dataA[m.indptrA[one_segment]:m.indptrA[one_segment + 1]] == 0).sum() == 1
    own = m.indicesA[m.indptrA[one_segment + 1]:m.indptrA[one_segment + 2]]
    assert len(set(gene[own])) == len(own) == 30
    assert (m.dataA == 0).any() and (p.w == 0).any()
    out = b""
    for model in MODELS:
        bound = q.tolerance(model)
        for sc in (None, scale):
            ref, explained = mchk.step(q, model, theta_in, sc)
            assert explained < int(p.w[p.has_bit].sum())                # some row with a weight has d = 0
            for tensors in (False, True):
                got, info = _quant(m, gene, G, model, tensors, scale=sc, theta_in=theta_in, max_iters=1, tol=0.0)
                qchk.agree(got, ref, bound)
                assert info["explained"] == explained and info["n_iter"] == 1
                assert abs(float(got.sum()) - explained) <= bound * explained
                out += got.tobytes()
        ref0, ex0 = mchk.step(q, model, p.aln(), scale)                 # from theta_0 = aln
        got, info = _quant(m, gene, G, model, False, scale=scale, max_iters=1, tol=0.0)
        qchk.agree(got, ref0, bound)
        assert info["explained"] == ex0 == p.W
        out += got.tobytes()
    return out


@pytest.mark.parametrize("H", EDGE_H)
def test_rows_columns_and_genes_around_the_thresholds(H):
    _bytes_of["edge%d" % H] = _edge_case(H)


@pytest.mark.parametrize("name,models,p,gene,G,theta", mchk.deviation_cases(), ids=[d[0] for d in mchk.deviation_cases()])
def test_the_rows_of_the_deviation_lose_no_mass(name, models, p, gene, G, theta):
    q = mchk.Grouping(p, gene, G)
    arrays = {"gene": ([0, 2, 3, 4], [0, 2, 1, 2], [3, 1, 3, 3]), "allele": ([0, 1, 2, 3], [0, 1, 2], [3, 3, 3]),
              "isoform": ([0, 2, 3, 4], [0, 1, 1, 2], [1, 3, 3, 3])}[name]
    m = _mat(2, 3, *arrays, [0, 3], [0, 1, 2], [10, 3, 5])
    assert qchk.Problem.of(m).bit_flat.tolist() == p.bit_flat.tolist() and qchk.Problem.of(m).w.tolist() == p.w.tolist()
    for model in MODELS:
        ref, explained = mchk.step(q, model, theta)
        lossy, _ = mchk.step(q, model, theta, reference_rule=True)
        for tensors in (False, True):
            got, info = _quant(m, gene, G, model, tensors, theta_in=theta, max_iters=1, tol=0.0)
            qchk.agree(got, ref, q.tolerance(model))
            assert info["explained"] == explained == 18 and abs(float(got.sum()) - 18.0) <= q.tolerance(model) * 18
            if model in models:
                assert float(lossy.sum()) < 17.0 < float(got.sum())


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------
FILL = 7.25


def _raw(m, gene, G, model, device=False, null_gene=False, theta_in=None):
    """ecb_quantify_model -- or, with ``device``, ecb_quantify_model_device on CUDA tensors -- on pre-filled outputs -> (rc, message, theta,
    (n_iter, delta, explained, converged))."""
    lib = ecb.load()
    arr = [np.ascontiguousarray(x, dtype=np.int32) for x in (m.indptrA, m.indicesA, m.dataA, m.indptrN, m.indicesN, m.dataN, gene)]
    T, H = m.num_loci, m.num_haplotypes
    theta = np.full((H, T), FILL)
    it, dl, ex, cv = C.c_uint32(77), C.c_double(FILL), C.c_int64(77), C.c_uint32(77)
    tin = None if theta_in is None else np.ascontiguousarray(theta_in, dtype=np.float64)
    fn, ptr = lib.ecb_quantify_model, ecb._ptr
    if device:
        import torch
        arr = [torch.from_numpy(v).cuda() for v in arr]
        tin = None if tin is None else torch.from_numpy(tin).cuda()
        theta = torch.full((H, T), FILL, dtype=torch.float64, device="cuda")
        fn, ptr = lib.ecb_quantify_model_device, ecb._dev_ptr
    rc = fn(0, len(arr[0]) - 1, T, H, len(arr[1]), ptr(arr[0]), ptr(arr[1]), ptr(arr[2]), len(arr[3]) - 1, len(arr[4]), ptr(arr[3]), ptr(arr[4]),
            ptr(arr[5]), -1, None, ptr(tin), 1, 0.0, G, None if null_gene else ptr(arr[6]), model, ptr(theta), C.byref(it), C.byref(dl), C.byref(ex),
            C.byref(cv))
    msg = lib.ecb_last_error(None).decode() if rc else ""
    if device:
        torch.cuda.synchronize()
        theta = theta.cpu().numpy()
    return rc, msg, theta, (it.value, dl.value, ex.value, cv.value)


def _untouched(theta, scalars):
    return bool(np.all(theta == FILL)) and scalars == (77, FILL, 77, 77)


def test_refusals_leave_the_outputs_untouched_and_the_next_call_works():
    m, q, z, scale = mchk.load_case(mchk.CASES[2])
    gene, G, T = q.gene, q.G, m.num_loci
    for device in (False, True):
        for model in (1, 2, 3, 4):
            for at, v in ((0, G), (T - 1, G), (T // 2, -1), (T - 1, -1), (3, 1 << 30)):
                bad = np.array(gene)
                bad[at] = v
                rc, msg, theta, scalars = _raw(m, bad, G, model, device)
                assert rc == -5 and "a gene id outside [0, n_genes)" in msg, (model, at, v, device, rc, msg)
                assert _untouched(theta, scalars), (model, at, v, device)
            rc, msg, theta, scalars = _raw(m, gene, G, model, device, null_gene=True)
            assert rc == -1 and _untouched(theta, scalars), (model, device, rc, msg)
            rc, msg, theta, scalars = _raw(m, gene, 0, model, device)
            assert rc == -1 and _untouched(theta, scalars), (model, device, rc, msg)
            # what ecb_quantify refuses, with its code
            nan = np.array(z["theta_0"])
            nan[0, 0] = np.nan
            rc, msg, theta, scalars = _raw(m, gene, G, model, device, theta_in=nan)
            assert rc == -5 and "an entry of theta_in is NaN, infinite or negative" in msg and _untouched(theta, scalars), (model, device, rc, msg)
        for model in (0, 5, 1 << 31):
            rc, msg, theta, scalars = _raw(m, gene, G, model, device)
            assert rc == -1 and "no such model" in msg and _untouched(theta, scalars), (model, device, rc, msg)
        # the call after the refusals: the device is unharmed
        for model in MODELS:
            rc, msg, theta, scalars = _raw(m, gene, G, model, device)
            assert rc == 0, msg
            ref, explained = mchk.step(q, model, z["theta_0"])
            qchk.agree(theta, ref, q.tolerance(model))
            assert scalars[0] == 1 and scalars[2] == explained and scalars[3] == 0


def test_the_empty_inputs_succeed():
    T, H = 5, 3
    gene, G = [0, 0, 1, 2, 2], 3
    for a in (([0], [], [], [0, 0], [], []), ([0, 0, 0, 0], [], [], [0, 2], [0, 2], [4, 1])):          # no row; rows, no non-zero
        m = _mat(H, T, *a)
        for model in MODELS:
            for tensors in (False, True):
                theta, info = _quant(m, gene, G, model, tensors)
                assert not theta.any() and info == {"n_iter": 0, "delta": 0.0, "explained": 0, "converged": True}
    # every weight 0: one step takes theta to 0 and the run has converged
    m = _mat(H, T, [0, 1, 3], [0, 1, 4], [1, 7, 2], [0, 0], [], [])
    for model in MODELS:
        theta, info = _quant(m, gene, G, model)
        assert not theta.any() and info == {"n_iter": 1, "delta": 0.0, "explained": 0, "converged": True}


# ---- 6. the command -----------------------------------------------------------------------------------------------------------------------
def test_the_command_writes_what_quantify_model_returns_and_reads_back_exactly(tmp_path):
    case = mchk.CASES[0]
    m, q, z, scale = mchk.load_case(case)
    src, grp, out = os.path.join(GOLDEN, case["ec"]), os.path.join(GOLDEN, case["grp"]), str(tmp_path / "o.tsv")
    env = dict(os.environ)
    env.pop("ALNTOOLS_GPUS", None)
    env["ALNTOOLS_TORCH"] = "0"
    r = subprocess.run([sys.executable, "-m", "alntools_amd.cli", "ecquant", src, out, "-v", "-M", "1", "-g", grp, "-i", "30", "-t", "1e-4"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    theta, info = _quant(m, q.gene, q.G, 1, max_iters=30, tol=1e-4)
    lines = open(out).read().splitlines()
    assert lines[0].split("\t") == ["locus"] + m.hname + ["total"] and [ln.split("\t")[0] for ln in lines[1:]] == m.lname
    back = np.array([[float(v) for v in ln.split("\t")[1:]] for ln in lines[1:]]).T
    assert back[:-1].tobytes() == theta.tobytes() and np.array_equal(back[-1], theta.sum(axis=0))
    assert "iterations: {:,};".format(info["n_iter"]) in r.stderr and "explained reads: {:,}".format(info["explained"]) in r.stderr
    assert "model 1, 401 genes" in r.stderr
    flat, _ = ecb.quantify(m.indptrA, m.indicesA, m.dataA, m.num_loci, m.num_haplotypes, m.indptrN, m.indicesN, m.dataN, max_iters=30, tol=1e-4)
    assert np.abs(theta - flat).max() > 1e-3                            # (not the flat model's answer)
    os.remove(out)
    r = subprocess.run([sys.executable, "-m", "alntools_amd.cli", "ecquant", src, out, "-M", "3"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 1 and "Error: model 3 needs a group file" in r.stderr and not os.path.exists(out)
