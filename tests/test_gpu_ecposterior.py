"""ecquant's posterior on the GPU (``ecb_posterior`` / ``ecb_posterior_device``) and the value-carrying transposition
(``ecb_csr_to_hapcsc_values*``): the device against the arrays recorded from the reference and against the checker
(``tests/post_checker.py``) for every case, model and recorded theta through both entry points; model 4 with and without a gene array; the
weighted sum of the posterior against one step of ``ecb.quantify`` / ``ecb.quantify_model``; determinism bit for bit (host entry, device
entry, a second call, a child process with the scratch poisoned); hand-built rows on both sides of every path switch; ``bit_ptr``; the
transposition's indptr / indices byte for byte and its payload as an exact permutation; every refusal with its outputs untouched; and the
command.

The bounds are derived in ``test_ecposterior.py`` (``post_checker.tolerance``): relative, entry by entry, the same entries 0; their terms
are computed from the matrix each test uses."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from alntools_amd import bin_utils, ecb, emase_h5

import post_checker as pchk
import quant_checker as qchk
import quant_model_checker as mchk
import test_gpu_ecquant_models as tgm
from test_ecquant_models import Q_LONG_GENE
from test_quant_constants import Q_LONG_ROW

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = pchk.GOLDEN
ALL_MODELS = (4, 1, 2, 3)


def _post(m, theta, scale=None, gene=None, G=0, model=4, tensors=False):
    """ecb.posterior over an ECMatrices -> (post, bit_ptr, row_mass) as numpy, through the host entry or, with CUDA tensors, the device one."""
    a = [m.indptrA, m.indicesA, m.dataA]
    if tensors:
        import torch
        a = [torch.as_tensor(np.asarray(x, dtype=np.int32), device="cuda") for x in a]
        theta, scale = (None if t is None else torch.as_tensor(np.asarray(t, dtype=np.float64), device="cuda") for t in (theta, scale))
        gene = None if gene is None else torch.as_tensor(np.asarray(gene, dtype=np.int32), device="cuda")
    out = ecb.posterior(a[0], a[1], a[2], m.num_loci, m.num_haplotypes, theta, scale=scale, gene=gene, n_genes=G, model=model)
    if tensors:
        assert all(t.is_cuda for t in out)
        out = tuple(t.cpu().numpy() for t in out)
    post, bit_ptr, mass = out
    assert post.dtype == np.float64 and bit_ptr.dtype == np.int64 and mass.dtype == np.float64
    assert bit_ptr.shape == (len(m.indicesA) + 1,) and mass.shape == (m.num_reads,) and post.shape == (int(bit_ptr[-1]),)
    return post, bit_ptr, mass


def _against_the_checker(m, q, lay, model, theta, scale, bound, mass_bound, tensors, gene=None, G=0):
    ref, ref_mass = pchk.posterior(q, lay, model, theta, scale)
    post, bit_ptr, mass = _post(m, theta, scale, gene, G, model, tensors)
    assert np.array_equal(bit_ptr, lay.bit_ptr)
    worst = qchk.agree(post, ref, bound)
    qchk.agree(mass, ref_mass, mass_bound)
    # a row nothing explains is all 0, every other row sums to 1
    dead = mass == 0
    sums = np.bincount(lay.bit_row, weights=post, minlength=lay.E)
    assert not sums[dead].any() and not post[dead[lay.bit_row]].any()
    return post, mass, worst


# ---- 1. the recorded arrays ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,model,k", pchk.TRIPLES, ids=pchk.TRIPLE_IDS)
def test_every_recorded_posterior_through_both_entry_points(case, model, k):
    r = pchk.load_case(case)
    bound, mass_bound = r.bound(model), pchk.tolerance(4, case["B"], r.p.H)
    theta = r.theta[(model, k)]
    for tensors in (False, True):
        post, mass, worst = _against_the_checker(r.m, r.grouping(model), r.lay, model, theta, r.scale, bound, mass_bound, tensors, r.gene, r.G)
        ref_worst = qchk.agree(r.recorded_of(post), r.ref[(model, k)], bound)
        print("%s model %d k=%d %s: worst relative difference %.3g of the reference's, %.3g of the checker's, bound %.3g"
              % (case["name"], model, k, "device" if tensors else "host", ref_worst, worst, bound))
        assert mass.all()                                                   # (every recorded row is explained)
        # the weighted sum is the recorded next theta, within the step's own bound
        qchk.agree(pchk.weighted_sum(r.p, r.lay, post), r.next[(model, k)], r.step_bound(model))


@pytest.mark.parametrize("case", pchk.CASES, ids=lambda c: c["name"])
def test_model_4_with_a_gene_array_is_model_4_without_one_byte_for_byte(case):
    r = pchk.load_case(case)
    gene, G = (r.gene, r.G) if r.gene is not None else (np.arange(r.m.num_loci) % 7, 7)
    theta = r.theta[(4, 5)]
    for tensors in (False, True):
        a = _post(r.m, theta, r.scale, None, 0, 4, tensors)
        b = _post(r.m, theta, r.scale, gene, G, 4, tensors)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("case,model,k", pchk.TRIPLES, ids=pchk.TRIPLE_IDS)
def test_the_weighted_sum_of_the_posterior_is_one_step_of_the_em(case, model, k):
    r = pchk.load_case(case)
    m, theta = r.m, r.theta[(model, k)]
    a = (m.indptrA, m.indicesA, m.dataA, m.num_loci, m.num_haplotypes, m.indptrN, m.indicesN, m.dataN)
    if model == 4:
        step, info = ecb.quantify(*a, scale=r.scale, theta_in=theta, max_iters=1, tol=0.0)
    else:
        step, info = ecb.quantify_model(*a, r.gene, r.G, model, scale=r.scale, theta_in=theta, max_iters=1, tol=0.0)
    post, _, mass = _post(m, theta, r.scale, r.gene, r.G, model)
    worst = qchk.agree(pchk.weighted_sum(r.p, r.lay, post), step, r.step_bound(model))
    print("%s model %d k=%d: the weighted sum against the step, worst relative difference %.3g, bound %.3g" % (case["name"], model, k, worst, r.step_bound(model)))
    assert info["explained"] == int(r.p.w[mass > 0].sum())


# ---- 2. the paths' edges ------------------------------------------------------------------------------------------------------------------
def _edge_case(H):
    """The matrix of ``test_gpu_ecquant_models._edge_matrix``: rows of Q_LONG_ROW and Q_LONG_ROW + 1 non-zeros, genes of Q_LONG_GENE and
    Q_LONG_GENE + 1 members, stored masks of 0 (one in the middle of a row, a whole row of them), empty rows, rows of weight 0, rows with
    d = 0 beside live ones.  Returns the bytes of everything the device returned."""
    m, gene, G, theta_in, scale, one_segment = tgm._edge_matrix(H)
    q = mchk.Grouping(qchk.Problem.of(m), gene, G)
    p, lay = q.p, pchk.Layout.of(m)
    lens = np.diff(m.indptrA)
    assert lens.max() == Q_LONG_ROW + 1 and (lens == Q_LONG_ROW).any() and (lens == 0).any()
    members = np.sort(np.bincount(gene))[::-1]
    assert members[:3].tolist() == [tgm.BIG, Q_LONG_GENE + 1, Q_LONG_GENE]
    row = m.dataA[m.indptrA[one_segment]:m.indptrA[one_segment + 1]]
    assert row[7] == 0 and row[6] != 0 and row[8] != 0                      # a stored mask of 0 in the middle of a row
    assert (p.w == 0).any() and m.num_haplotypes == H
    out = b""
    for model in ALL_MODELS:
        bound, mass_bound = pchk.tolerance(model, p.B, H, q.M, q.R), pchk.tolerance(4, p.B, H)
        for sc in (None, scale):
            for tensors in (False, True):
                post, mass, _ = _against_the_checker(m, q, lay, model, theta_in, sc, bound, mass_bound, tensors, gene, G)
                # row_mass says which rows nothing explains: rows 5 and 750 (theta = 0 on all their targets) among the live ones
                assert mass[5] == 0 and mass[750] == 0 and lens[5] > 0 and (p.has_bit & (mass == 0)).any() and (mass > 0).sum() > 1000
                # a row of weight 0 gets its posterior like any other
                e = int(np.flatnonzero((p.w == 0) & (mass > 0))[0])
                assert abs(post[lay.bit_row == e].sum() - 1.0) <= bound + p.B * 2.0 ** -52
                out += post.tobytes() + mass.tobytes()
    return out


EDGE_H = [1, 8, 31]
_bytes_of = {}


def _kept(key, make):
    if key not in _bytes_of:
        _bytes_of[key] = make()
    return _bytes_of[key]


@pytest.mark.parametrize("H", EDGE_H)
def test_rows_and_genes_around_the_thresholds(H):
    _bytes_of["edge%d" % H] = _edge_case(H)


@pytest.mark.parametrize("name,models,p,gene,G,theta", mchk.deviation_cases(), ids=[d[0] for d in mchk.deviation_cases()])
def test_the_rows_of_the_deviation_keep_their_whole_mass(name, models, p, gene, G, theta):
    """The three hand-built matrices of ``test_gpu_ecquant_models.py`` (H = 2, gene A = {t0, t1}, gene B = {t2}; row 0 touches a member
    whose own D is 0 while its Phi is positive), rebuilt here: the member is left out of the denominator, so row 0 still sums to 1."""
    arrays = {"gene": ([0, 2, 3, 4], [0, 2, 1, 2], [3, 1, 3, 3]), "allele": ([0, 1, 2, 3], [0, 1, 2], [3, 3, 3]),
              "isoform": ([0, 2, 3, 4], [0, 1, 1, 2], [1, 3, 3, 3])}[name]
    m = tgm._mat(2, 3, *arrays, [0, 3], [0, 1, 2], [10, 3, 5])
    assert qchk.Problem.of(m).bit_flat.tolist() == p.bit_flat.tolist()
    q, lay = mchk.Grouping(p, gene, G), pchk.Layout.of(m)
    for model in (1, 2, 3):
        bound = pchk.tolerance(model, p.B, 2, q.M, q.R)
        for tensors in (False, True):
            post, mass, _ = _against_the_checker(m, q, lay, model, theta, None, bound, pchk.tolerance(4, p.B, 2), tensors, gene, G)
            sums = np.bincount(lay.bit_row, weights=post, minlength=3)
            assert np.all(np.abs(sums - 1.0) <= bound + p.B * 2.0 ** -52) and mass.all()
            qchk.agree(pchk.weighted_sum(p, lay, post), mchk.step(q, model, theta)[0], q.tolerance(model))
            if model in models:                                             # the reference's rule loses this share of row 0
                lossy = mchk.step(q, model, theta, reference_rule=True)[0]
                assert float(lossy.sum()) < 17.0 < float(pchk.weighted_sum(p, lay, post).sum())


# ---- 3. determinism -----------------------------------------------------------------------------------------------------------------------
def _determinism(case, model):
    """Host entry, device entry and a second call: all bit for bit.  Returns the bytes compared."""
    r = pchk.load_case(case)
    theta = r.theta[(model, 5)]
    a = _post(r.m, theta, r.scale, r.gene, r.G, model, False)
    b = _post(r.m, theta, r.scale, r.gene, r.G, model, False)
    d = _post(r.m, theta, r.scale, r.gene, r.G, model, True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), "two calls differ"
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, d)), "host and device entry differ"
    return b"".join(x.tobytes() for x in a)


DET = [(c, model) for c in pchk.CASES for model in c["models"]]
DET_IDS = ["%s-m%d" % (c["name"], model) for c, model in DET]


@pytest.mark.parametrize("case,model", DET, ids=DET_IDS)
def test_both_entries_and_a_second_call_agree_bit_for_bit(case, model):
    _bytes_of[(case["name"], model)] = _determinism(case, model)


def _values_case(key):
    m, payload, lay = _conv(key)
    host = ecb.csr_to_hapcsc_values_host(m.indptrA, m.indicesA, m.dataA, payload, m.num_loci, m.num_haplotypes)
    return b"".join(np.ascontiguousarray(x).tobytes() for x in host)


def _digest():
    h = hashlib.sha256()
    for case, model in DET:
        h.update(_kept((case["name"], model), lambda: _determinism(case, model)))
    for H in EDGE_H:
        h.update(_kept("edge%d" % H, lambda: _edge_case(H)))
    for key in CONV:
        h.update(_kept("conv-" + key, lambda: _values_case(key)))
    return h.hexdigest()


def test_everything_once_more_with_the_scratch_poisoned_gives_the_same_bits():
    """One fresh child process with ECB_POISON_SCRATCH=1: every buffer the library allocates is filled with 0x01 first, so a pass that
    relied on fresh memory being 0 gives other bits than this process, whose digest of the same calls the child's must equal."""
    env = dict(os.environ)
    env["ECB_POISON_SCRATCH"] = "1"
    env["ALNTOOLS_TORCH"] = "1"
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_ecposterior as t; print('digest', t._digest())" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "digest " + _digest() in r.stdout


# ---- 4. the transposition with a payload --------------------------------------------------------------------------------------------------
CONV = ("c1", "h8", "edge31", "longcol")


def _conv(key):
    """(matrix, payload, layout).  The payload: distinct integers as floats, so that a misplaced value cannot hide.  ``longcol``: one column
    that every row holds (longer than any block of the emit pass) beside sparse ones; ``edge31``: 31 haplotypes, rows longer than Q_LONG_ROW."""
    def make():
        if key in ("c1", "h8"):
            m = pchk.load_case([c for c in pchk.CASES if c["name"] == key][0]).m
        elif key == "edge31":
            m = tgm._edge_matrix(31)[0]
            keep = m.dataA != 0                                             # (the conversion refuses a stored mask of 0)
            row = np.repeat(np.arange(m.num_reads), np.diff(m.indptrA))[keep]
            m = tgm._mat(31, m.num_loci, np.concatenate([[0], np.cumsum(np.bincount(row, minlength=m.num_reads))]), m.indicesA[keep], m.dataA[keep],
                         m.indptrN, m.indicesN, m.dataN)
        else:
            rng = np.random.default_rng(5)
            E, T, H = 3000, 50, 5
            rows = [np.unique(np.concatenate([[17], rng.choice(T, size=int(rng.integers(0, 4)), replace=False)])) for _ in range(E)]
            ix = np.concatenate(rows)
            m = tgm._mat(H, T, np.cumsum([0] + [len(x) for x in rows]), ix, rng.integers(1, 1 << H, size=len(ix)), [0, 1], [0], [1])
        lay = pchk.Layout.of(m)
        return m, np.arange(lay.n_bits, dtype=np.float64) * 3.0 + 1.0, lay
    return _kept(("post-conv", key), make)


@pytest.mark.parametrize("key", CONV)
def test_the_value_carrying_transposition_moves_every_value_to_its_entry(key):
    import torch
    m, payload, lay = _conv(key)
    T, H = m.num_loci, m.num_haplotypes
    if key == "longcol":
        assert np.bincount(m.indicesA, minlength=T)[17] == m.num_reads > 1024
    cptr, cidx = ecb.csr_to_hapcsc_host(m.indptrA, m.indicesA, m.dataA, T, H)
    assert np.array_equal(cptr, lay.csc_indptr) and np.array_equal(cidx, lay.csc_indices)          # (the checker's layout is the conversion's)
    want = lay.to_csc(payload)
    host = ecb.csr_to_hapcsc_values_host(m.indptrA, m.indicesA, m.dataA, payload, T, H)
    dev = ecb.csr_to_hapcsc_values(*(torch.as_tensor(np.asarray(x, dtype=np.int32), device="cuda") for x in (m.indptrA, m.indicesA, m.dataA)),
                                   torch.as_tensor(payload, device="cuda"), T, H)
    dev = tuple(t.cpu().numpy() for t in dev)
    for got in (host, dev):
        assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.float64
        assert got[0].tobytes() == cptr.tobytes() and got[1].tobytes() == cidx.tobytes()
        assert got[2].tobytes() == want.tobytes()
        assert np.array_equal(np.sort(got[2]), payload)                     # an exact permutation
        assert np.array_equal(lay.from_csc(got[2]), payload)
    _bytes_of["conv-" + key] = b"".join(np.ascontiguousarray(x).tobytes() for x in host)
    # the count-only call, and the incidence-only conversion after it: unchanged
    tot = C.c_uint64()
    assert ecb.load().ecb_csr_to_hapcsc_values(0, m.num_reads, T, H, ecb._ptr(m.indptrA), ecb._ptr(m.indicesA), ecb._ptr(m.dataA), None, None, None,
                                               None, 0, C.byref(tot)) == 0 and tot.value == lay.n_bits
    again = ecb.csr_to_hapcsc_host(m.indptrA, m.indicesA, m.dataA, T, H)
    assert again[0].tobytes() == cptr.tobytes() and again[1].tobytes() == cidx.tobytes()


def test_the_transposition_refuses_what_the_incidence_only_one_refuses():
    import torch
    m, payload, lay = _conv("c1")
    T, H, E = m.num_loci, m.num_haplotypes, m.num_reads
    lib = ecb.load()
    falling = np.array(m.indptrA)
    falling[100], falling[101] = m.indptrA[101] + 1, m.indptrA[100]
    zero = np.array(m.dataA)
    zero[7] = 0
    far = np.array(m.indicesA)
    far[3] = T
    for what, (ip, ix, da), va in (("ptr", (falling, m.indicesA, m.dataA), payload), ("mask 0", (m.indptrA, m.indicesA, zero), payload),
                                   ("locus", (m.indptrA, far, m.dataA), payload), ("no values", (m.indptrA, m.indicesA, m.dataA), None)):
        code = -1 if va is None else -5
        ip, ix, da = (np.ascontiguousarray(x, dtype=np.int32) for x in (ip, ix, da))
        cp, ci, cd = np.full((H, T + 1), 77, dtype=np.int32), np.full(lay.n_bits, 77, dtype=np.int32), np.full(lay.n_bits, 7.25)
        tot = C.c_uint64()
        rc = lib.ecb_csr_to_hapcsc_values(0, E, T, H, ecb._ptr(ip), ecb._ptr(ix), ecb._ptr(da), ecb._ptr(va), ecb._ptr(cp), ecb._ptr(ci), ecb._ptr(cd),
                                          lay.n_bits, C.byref(tot))
        assert rc == code, (what, rc, lib.ecb_last_error(None))
        assert (cp == 77).all() and (ci == 77).all() and (cd == 7.25).all(), what
        d = [torch.from_numpy(x).cuda() for x in (ip, ix, da)]
        dv = None if va is None else torch.from_numpy(va).cuda()
        o = [torch.full((H, T + 1), 77, dtype=torch.int32, device="cuda"), torch.full((lay.n_bits,), 77, dtype=torch.int32, device="cuda"),
             torch.full((lay.n_bits,), 7.25, dtype=torch.float64, device="cuda")]
        rc = lib.ecb_csr_to_hapcsc_values_device(0, E, T, H, *(ecb._dev_ptr(t) for t in d), ecb._dev_ptr(dv), *(ecb._dev_ptr(t) for t in o), C.byref(tot))
        torch.cuda.synchronize()
        assert rc == code, (what, rc, lib.ecb_last_error(None))
        assert bool((o[0] == 77).all()) and bool((o[1] == 77).all()) and bool((o[2] == 7.25).all()), what
    # too little room: ECB_ERR_ARG, *total says how much
    cp, ci, cd = np.full((H, T + 1), 77, dtype=np.int32), np.full(lay.n_bits, 77, dtype=np.int32), np.full(lay.n_bits, 7.25)
    tot = C.c_uint64()
    rc = lib.ecb_csr_to_hapcsc_values(0, E, T, H, ecb._ptr(m.indptrA), ecb._ptr(m.indicesA), ecb._ptr(m.dataA), ecb._ptr(payload), ecb._ptr(cp), ecb._ptr(ci),
                                      ecb._ptr(cd), lay.n_bits - 1, C.byref(tot))
    assert rc == -1 and tot.value == lay.n_bits and (cp == 77).all() and (ci == 77).all() and (cd == 7.25).all()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------
FILL = 7.25


def _raw(m, theta, gene, G, model, device=False, scale=None, n_bits=None, null=(), arrays=None, sizes=None):
    """ecb_posterior -- or, with ``device``, ecb_posterior_device on CUDA tensors -- on pre-filled outputs -> (rc, message, post, bit_ptr,
    row_mass).  ``null``: the names of the pointers handed over as NULL.  ``sizes``: n_ecs, n_loci, n_haps or nnz other than the matrix's
    own, for the refusals that look at nothing else."""
    lib = ecb.load()
    ip, ix, da = (np.ascontiguousarray(x, dtype=np.int32) for x in (arrays or (m.indptrA, m.indicesA, m.dataA)))
    T, H = m.num_loci, m.num_haplotypes
    lay_bits = int(np.unpackbits(np.ascontiguousarray(m.dataA, dtype=np.int32).view(np.uint8)).sum())
    v = {"ip": ip, "ix": ix, "da": da, "scale": None if scale is None else np.ascontiguousarray(scale, dtype=np.float64),
         "theta": np.ascontiguousarray(theta, dtype=np.float64), "gene": None if gene is None else np.ascontiguousarray(gene, dtype=np.int32),
         "post": np.full(lay_bits, FILL), "bit_ptr": np.full(len(ix) + 1, 77, dtype=np.int64), "mass": np.full(len(ip) - 1, FILL)}
    fn, ptr = lib.ecb_posterior, ecb._ptr
    if device:
        import torch
        v = {k: None if a is None else torch.from_numpy(a).cuda() for k, a in v.items()}
        fn, ptr = lib.ecb_posterior_device, ecb._dev_ptr
    p = {k: None if k in null else ptr(a) for k, a in v.items()}
    z = dict({"n_ecs": len(ip) - 1, "n_loci": T, "n_haps": H, "nnz": len(ix)}, **(sizes or {}))
    rc = fn(0, z["n_ecs"], z["n_loci"], z["n_haps"], z["nnz"], p["ip"], p["ix"], p["da"], p["scale"], p["theta"], G, p["gene"], model,
            lay_bits if n_bits is None else n_bits, p["post"], p["bit_ptr"], p["mass"])
    msg = lib.ecb_last_error(None).decode() if rc else ""
    if device:
        torch.cuda.synchronize()
        v = {k: None if a is None else a.cpu().numpy() for k, a in v.items()}
    return rc, msg, v["post"], v["bit_ptr"], v["mass"]


def _untouched(post, bit_ptr, mass):
    return bool(np.all(post == FILL)) and bool(np.all(bit_ptr == 77)) and bool(np.all(mass == FILL))


def test_refusals_leave_the_outputs_untouched_and_the_next_call_works():
    r = pchk.load_case([c for c in pchk.CASES if c["name"] == "ms"][0])
    m, gene, G, T = r.m, r.gene, r.G, r.m.num_loci
    theta = r.theta[(4, 0)]
    n_bits = r.lay.n_bits
    falling = np.array(m.indptrA)
    falling[100], falling[101] = m.indptrA[101] + 1, m.indptrA[100]
    wide = np.array(m.dataA)
    wide[11] = 1 << m.num_haplotypes
    unsorted = np.array(m.indicesA)
    e = int(np.flatnonzero(np.diff(m.indptrA) >= 2)[0])
    unsorted[m.indptrA[e]], unsorted[m.indptrA[e] + 1] = m.indicesA[m.indptrA[e] + 1], m.indicesA[m.indptrA[e]]
    for device in (False, True):
        for model in (1, 2, 3, 4):
            def refused(code, text, **kw):
                rc, msg, post, bit_ptr, mass = _raw(m, kw.pop("theta", theta), kw.pop("gene", gene), kw.pop("G", G), kw.pop("model", model), device, **kw)
                assert rc == code and text in msg, (model, device, kw, rc, msg)
                assert _untouched(post, bit_ptr, mass), (model, device, kw)
            # what ecb_quantify_model refuses on A, scale, gene and model, with its codes
            refused(-5, "malformed CSR", arrays=(falling, m.indicesA, m.dataA))
            refused(-5, "malformed CSR", arrays=(m.indptrA, m.indicesA, wide))
            refused(-5, "columns not strictly ascending", arrays=(m.indptrA, unsorted, m.dataA))
            bad = np.ones((m.num_haplotypes, T))
            bad[1, T // 2] = -1.0
            refused(-5, "an entry of scale is NaN, infinite or negative", scale=bad)
            for at, v in ((0, G), (T - 1, -1), (3, 1 << 30)):
                g2 = np.array(gene)
                g2[at] = v
                refused(-5, "a gene id outside [0, n_genes)", gene=g2)
            refused(-1, "", G=0)
            if model != 4:
                refused(-1, "no gene array", null=("gene",))
            # theta: a text of its own
            for v in (np.nan, np.inf, -1.0):
                t2 = np.array(theta)
                t2[0, 3] = v
                refused(-5, "ecposterior: an entry of theta is NaN, infinite or negative", theta=t2)
            refused(-1, "no theta", null=("theta",))
            refused(-1, "no post", null=("post",))
            for nb in (n_bits - 1, n_bits + 1, 0):
                refused(-1, "n_bits is %d, the matrix has %d set bits" % (nb, n_bits), n_bits=nb, **({"null": ("post",)} if nb == 0 else {}))
        for model in (0, 5, 1 << 31):
            rc, msg, post, bit_ptr, mass = _raw(m, theta, gene, G, model, device)
            assert rc == -1 and "no such model" in msg and _untouched(post, bit_ptr, mass), (model, device, rc, msg)
        # the call after the refusals: the device is unharmed; the optional outputs may be NULL
        for model in ALL_MODELS:
            ref, ref_mass = pchk.posterior(r.grouping(model), r.lay, model, theta)
            rc, msg, post, bit_ptr, mass = _raw(m, theta, gene, G, model, device)
            assert rc == 0, msg
            qchk.agree(post, ref, r.bound(model))
            assert np.array_equal(bit_ptr, r.lay.bit_ptr) and mass.all()
            rc, msg, post2, bit_ptr, mass = _raw(m, theta, gene, G, model, device, null=("bit_ptr", "mass"))
            assert rc == 0 and post2.tobytes() == post.tobytes() and bool(np.all(bit_ptr == 77)) and bool(np.all(mass == FILL))


def test_sizes_beyond_the_limits_are_refused_before_anything_is_read():
    """What ``ecb_quantify_model`` refuses on the sizes of A and of the grouping, with its codes (``qp_check_args``: no pointer is followed,
    nothing is allocated), through both entry points, every output as it was."""
    r = pchk.load_case([c for c in pchk.CASES if c["name"] == "ms"][0])
    m, gene, G, H = r.m, r.gene, r.G, r.m.num_haplotypes
    theta = r.theta[(4, 0)]
    LIMIT, ARG = -8, -1
    for device in (False, True):
        for model in ALL_MODELS:
            for code, text, kw in (
                    (LIMIT, "2^30 non-zeros or more", dict(sizes={"nnz": 1 << 30})),
                    (LIMIT, "haplotypes x loci does not fit 31 bits", dict(sizes={"n_loci": (1 << 31) // H + 1})),
                    (LIMIT, "haplotypes x loci does not fit 31 bits", dict(sizes={"n_loci": (1 << 31) // 31 + 1, "n_haps": 31})),
                    (LIMIT, "haplotypes x genes does not fit 31 bits", dict(G=(1 << 31) // H + 1)),
                    (LIMIT, "int32 limits", dict(sizes={"n_ecs": (1 << 31) - 1})),
                    (LIMIT, "int32 limits", dict(sizes={"n_ecs": (1 << 32) - 1})),
                    (ARG, "bad argument", dict(sizes={"n_haps": 32})),
                    (ARG, "bad argument", dict(sizes={"n_haps": 0})),
                    (ARG, "bad argument", dict(sizes={"n_loci": 0})),
                    (ARG, "bad argument", dict(null=("ip",))),
                    (ARG, "bad argument", dict(null=("ix",))),
                    (ARG, "bad argument", dict(null=("da",)))):
                kw = dict(kw)
                rc, msg, post, bit_ptr, mass = _raw(m, theta, gene, kw.pop("G", G), model, device, **kw)
                assert rc == code and text in msg, (model, device, kw, rc, msg)
                assert _untouched(post, bit_ptr, mass), (model, device, kw)
        # the sizes just below the limits pass the argument check: the refusal is then the matrix's (its row pointers do not end at nnz)
        rc, msg, post, bit_ptr, mass = _raw(m, theta, gene, G, 4, device, sizes={"nnz": len(m.indicesA) - 1})
        assert rc == -5 and "malformed CSR" in msg and _untouched(post, bit_ptr, mass)
        # model 4 without a gene array takes any n_genes
        rc, msg, post, bit_ptr, mass = _raw(m, theta, None, (1 << 31) // H + 1, 4, device)
        assert rc == 0, msg


def test_2_to_the_32_set_bits_are_refused_on_the_device():
    """H = 31, 8 457 rows that each hold all 16 384 targets with the mask 0x7FFFFFFF: 138 559 488 non-zeros, 4 295 344 128 set bits, the first
    multiple of a row above 2^32.  The count is the device's (the scan's 64-bit total); the refusal comes before ``n_bits`` is compared, so
    ``n_bits = 0`` and no ``post`` will do.  One row less is below the limit, and is then refused for its ``n_bits`` with both numbers."""
    import torch
    lib = ecb.load()
    H, T, E = 31, 1 << 14, 8457
    assert E * T * H >= 1 << 32 > (E - 1) * T * H and E * T < 1 << 30
    ip = torch.arange(E + 1, dtype=torch.int64, device="cuda").mul_(T).to(torch.int32)
    ix = torch.arange(T, dtype=torch.int32, device="cuda").repeat(E)
    da = torch.full((E * T,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    theta = torch.ones((H, T), dtype=torch.float64, device="cuda")
    bit_ptr = torch.full((E * T + 1,), 77, dtype=torch.int64, device="cuda")
    mass = torch.full((E,), FILL, dtype=torch.float64, device="cuda")
    P = ecb._dev_ptr
    try:
        for rows, code, text in ((E, -8, "more than 2^32-1 set haplotype bits"),
                                 (E - 1, -1, "n_bits is 0, the matrix has %d set bits" % ((E - 1) * T * H))):
            rc = lib.ecb_posterior_device(0, rows, T, H, rows * T, P(ip), P(ix), P(da), None, P(theta), 0, None, 4, 0, None, P(bit_ptr), P(mass))
            torch.cuda.synchronize()
            assert rc == code and text in lib.ecb_last_error(None).decode(), (rows, rc, lib.ecb_last_error(None))
            assert bool((bit_ptr == 77).all()) and bool((mass == FILL).all())
    finally:
        del ip, ix, da, bit_ptr
        assert lib.ecb_release_scratch(0) == 0          # (the library's pool grew to this matrix: given back)


def test_the_empty_inputs_write_bit_ptr_alone():
    T, H = 5, 3
    gene, G = [0, 0, 1, 2, 2], 3
    theta = np.ones((H, T))
    for a in (([0], [], []), ([0, 0, 0, 0], [], [])):                      # no row; rows, no non-zero
        m = tgm._mat(H, T, *a, [0, 0], [], [])
        for model in ALL_MODELS:
            for device in (False, True):
                rc, msg, post, bit_ptr, mass = _raw(m, theta, gene, G, model, device)
                assert rc == 0 and bit_ptr.tolist() == [0] and len(post) == 0 and bool(np.all(mass == FILL)), (model, device, msg)
    # a matrix whose every stored mask is 0: no bits, no values, every row's mass 0
    m = tgm._mat(H, T, [0, 1, 3], [0, 1, 4], [0, 0, 0], [0, 0], [], [])
    for model in ALL_MODELS:
        for tensors in (False, True):
            post, bit_ptr, mass = _post(m, theta, None, gene, G, model, tensors)
            assert len(post) == 0 and bit_ptr.tolist() == [0, 0, 0, 0] and mass.tolist() == [0.0, 0.0]


# ---- 6. the command -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [4, 2])
def test_the_command_writes_the_posterior_at_the_theta_it_writes(tmp_path, model):
    case = [c for c in pchk.CASES if c["name"] == "c1"][0]
    r = pchk.load_case(case)
    m = r.m
    src, grp = os.path.join(GOLDEN, case["ec"]), os.path.join(GOLDEN, case["grp"])
    plain, out, h5 = str(tmp_path / "plain.tsv"), str(tmp_path / "out.tsv"), str(tmp_path / "out.h5")
    env = dict(os.environ)
    env.pop("ALNTOOLS_GPUS", None)
    env["ALNTOOLS_TORCH"] = "0"
    more = ["-M", "2", "-g", grp] if model == 2 else []
    for args in ([src, plain], [src, out, "-w", h5]):
        run = subprocess.run([sys.executable, "-m", "alntools_amd.cli", "ecquant"] + args + more + ["-i", "30", "-t", "1e-4"], cwd=ROOT, env=env,
                             capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stderr[-2000:]
    assert open(out, "rb").read() == open(plain, "rb").read()               # the table is the run's without -w, byte for byte
    lines = open(out).read().splitlines()
    theta = np.array([[float(v) for v in ln.split("\t")[1:-1]] for ln in lines[1:]]).T
    post = _post(m, theta, None, r.gene, r.G, model)[0]
    got = emase_h5.load_values(h5)
    assert len(got) == m.num_haplotypes
    start = 0
    for h, (ip, ix, data) in enumerate(got):
        n = len(ix)
        assert np.array_equal(ip, r.lay.csc_indptr[h]) and np.array_equal(ix, r.lay.csc_indices[start:start + n])
        assert data.dtype == np.float64 and data.tobytes() == r.lay.to_csc(post)[start:start + n].tobytes()
        start += n
    assert start == r.lay.n_bits
    # emase2ec of the file returns the .bin's A (and its N, names and lengths)
    back = str(tmp_path / "back.bin")
    bin_utils.emase2ec(h5, back)
    assert open(back, "rb").read() == open(src, "rb").read()
    # a run that fails leaves neither file
    os.remove(out); os.remove(h5)
    run = subprocess.run([sys.executable, "-m", "alntools_amd.cli", "ecquant", src, out, "-w", h5, "-s", "nobody"], cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=300)
    assert run.returncode == 1 and "Error: sample nobody is not in" in run.stderr and not os.path.exists(out) and not os.path.exists(h5)
