"""ecboot on the GPU (``ecb_resample*`` / ``ecb_quantify_bootstrap*``) against ``tests/boot_checker.py``: the replicates byte for byte through
both entry points, on the golden files and on synthetic N at every edge of the draw kernel; the bootstrap as the composition it is defined as
(``ecb.quantify_cells`` / ``ecb.quantify_cells_model`` on the resampled N, byte for byte), its moments against the checker's Welford loop,
one rule for every route, every refusal with its outputs untouched, and the command.

The bound of the moments.  The device and the checker run the same loop over the same ``reps``; they differ where ``hipcc`` contracts
``M + d * (x - m)`` to one FMA.  With ``X = max_b |x_b|`` of an entry, every ``d`` and ``x - m`` is at most ``X`` in size (all ``x_b >= 0``,
``m`` between their extremes up to rounding).  A step of the mean takes three roundings (``x - m``, ``/ (b + 1)``, ``m +``), each at most
``2^-53`` of a quantity no larger than ``X``: after ``B`` steps either side is within ``3 B 2^-53 X`` of the exact mean recurrence, the two
sides within ``3 B 2^-52 X`` of each other.  A step of ``M`` adds ``p = d (x - m')``: ``d`` and ``x - m'`` inherit the error of ``m``
(at most ``3 B 2^-53 X`` each, against factors at most ``X``) and add a rounding each, the product and the sum one more each (the FMA one
fewer): ``|error of p| <= (6 B + 3) 2^-53 X^2``, and the running sum, at most ``B X^2``, rounds by at most ``B 2^-53 X^2`` per step.  Over
``B`` steps one side is within ``(7 B + 3) B 2^-53 X^2``, the two sides within ``(7 B + 3) x B 2^-52 X^2`` of each other: the multiples of
``B 2^-52`` are 3 for the mean and ``7 B + 3`` for ``M``.  ``sd`` is compared as ``M = sd^2 (B - 1)``: the root, the division and the
square back add ``3 x 2^-52`` relative to ``M <= B X^2``.  The totals: the same with ``Y = max_b y_b``.  (Measured on the device:
DESIGN.md section 7, ecboot.)"""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from alntools_amd import bin_utils, ecb, ecb_boot

import boot_checker as bc
from test_ecboot import BS_WG_DRAWS, C1, GOLDEN, MS, load, weights_of

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GRP = os.path.join(GOLDEN, "quant_model_c1.grp.txt")
INFO = ("n_iter", "delta", "explained", "converged")
ARG, CONTRACT, LIMIT = -1, -5, -8
EPS = 2.0 ** -52
_kept = {}


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def _dev(a, dt):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device="cuda")


def _resample(n_ecs, pn, xn, dn, tensors, **kw):
    if tensors:
        pn, xn, dn = (_dev(a, np.int32) for a in (pn, xn, dn))
    out = ecb_boot.resample(n_ecs, pn, xn, dn, **kw)
    if tensors:
        assert all(t.is_cuda for t in out)
    out = tuple(_np(t) for t in out)
    assert all(a.dtype == np.int32 for a in out)
    return out


def _one_column(idx, cnt):
    return np.array([0, len(idx)], dtype=np.int32), np.asarray(idx, dtype=np.int32), np.asarray(cnt, dtype=np.int32)


def _dense(w):
    rows = np.arange(len(w))
    return _one_column(rows, w)


def _heavy():
    w = np.ones(3001, dtype=np.int64)
    w[1500] = 100000
    return w


def _spread(W, E=5):
    """W reads over E rows, unevenly, a weightless row among them."""
    w = np.zeros(E, dtype=np.int64)
    w[0], w[2], w[E - 1] = W // 2, W // 3, W - W // 2 - W // 3
    return w


#: name -> (n_ecs, (indptr_n, indices_n, data_n), replicates)
SYNTH = {
    "W1": (3, _dense([0, 1, 0]), 4),
    "W2": (2, _dense([1, 1]), 4),
    "W-odd": (3, _dense([3, 0, 4]), 4),
    "W-wg-1": (5, _dense(_spread(BS_WG_DRAWS - 1)), 2),
    "W-wg": (5, _dense(_spread(BS_WG_DRAWS)), 2),
    "W-wg+1": (5, _dense(_spread(BS_WG_DRAWS + 1)), 2),
    "E1": (1, _dense([37]), 3),
    "zeros-first-last-between": (7, _dense([0, 0, 5, 0, 3, 0, 0]), 4),
    "W5-over-7": (7, _dense([1, 0, 1, 1, 0, 1, 1]), 256),
    "W-below-G": (100, _one_column([3, 50, 51, 99], [1, 2, 3, 4]), 3),
    "heavy-row": (3001, _dense(_heavy()), 2),
    "two-heavy-rows": (4, _dense([30000, 0, 30001, 0]), 2),
    "listed-twice": (3, _one_column([0, 2, 0], [3, 4, 5]), 4),
    "E-off-the-block": (1000, _dense(np.random.default_rng(5).integers(0, 4, size=1000)), 3),
}
# W = 2^k and 2^k +- 1 around the guide's shift: 8 rows, G = 8 -- shift 0 up to W = 8, 1 up to 16, 2 from 17 on
for _W in (7, 8, 9, 15, 16, 17):
    SYNTH["guide-W%d" % _W] = (8, _dense(_spread(_W, 8)), 3)


@pytest.mark.parametrize("name", sorted(SYNTH))
def test_synthetic_n_at_the_draw_kernels_edges_byte_for_byte(name):
    n_ecs, (pn, xn, dn), B = SYNTH[name]
    w = bc.weights(n_ecs, pn, xn, dn)
    assert (np.asarray(dn) >= 0).all()
    ptr, ec, cnt, dense = bc.resample(w, 11, 5, B)
    assert (dense.sum(axis=1) == w.sum()).all() and not dense[:, w == 0].any()
    if name == "W5-over-7":
        seen = set()
        for b in range(5, 5 + B):
            seen |= set(bc.xs(11, b, 5).tolist())
        assert seen == {0, 1, 2, 3, 4}
    if name.startswith("guide-W"):
        assert int(w.sum()) == int(name[7:])
    for tensors in (False, True):
        got = _resample(n_ecs, pn, xn, dn, tensors, seed=11, b0=5, n_reps=B)
        assert got[0].tobytes() == ptr.tobytes() and got[1].tobytes() == ec.tobytes() and got[2].tobytes() == cnt.tobytes(), (name, tensors)


def _golden(path, sample, B, seed=3):
    key = ("golden", path, sample, B, seed)
    if key not in _kept:
        _kept[key] = bc.resample(weights_of(path, sample), seed, 0, B)
    return _kept[key]


@pytest.mark.parametrize("path,sample,B", [(C1, None, 8), (MS, None, 2), (MS, 3, 2)], ids=["g2_c1", "g4b-pooled", "g4b-sample3"])
def test_the_golden_files_replicates_byte_for_byte_through_both_entry_points(path, sample, B):
    m = load(path)
    ptr, ec, cnt, dense = _golden(path, sample, B)
    assert ptr[-1] > 0
    for tensors in (False, True):
        got = _resample(m.num_reads, m.indptrN, m.indicesN, m.dataN, tensors, sample=sample, seed=3, n_reps=B)
        assert got[0].tobytes() == ptr.tobytes() and got[1].tobytes() == ec.tobytes() and got[2].tobytes() == cnt.tobytes()


def test_a_replicate_does_not_depend_on_which_others_are_drawn():
    m = load(C1)
    ptr, ec, cnt, _ = _golden(C1, None, 8)
    got = _resample(m.num_reads, m.indptrN, m.indicesN, m.dataN, False, seed=3, b0=3, n_reps=2)
    a, z = int(ptr[3]), int(ptr[5])
    assert np.array_equal(got[0], ptr[3:6] - ptr[3]) and np.array_equal(got[1], ec[a:z]) and np.array_equal(got[2], cnt[a:z])
    # the last replicate number there is
    last = _resample(m.num_reads, m.indptrN, m.indicesN, m.dataN, True, seed=3, b0=(1 << 32) - 1, n_reps=1)
    want = bc.resample(weights_of(C1), 3, (1 << 32) - 1, 1)
    assert all(np.array_equal(g, w) for g, w in zip(last, want[:3]))
    none = _resample(m.num_reads, m.indptrN, m.indicesN, m.dataN, False, seed=3, n_reps=0)
    assert none[0].tolist() == [0] and len(none[1]) == 0


def test_a_capacity_that_is_too_small_writes_the_pointers_and_the_size_only():
    import torch
    m = load(C1)
    ptr, ec, cnt, _ = _golden(C1, None, 8)
    lib = ecb_boot.load()
    pn, xn, dn = (np.ascontiguousarray(a, dtype=np.int32) for a in (m.indptrN, m.indicesN, m.dataN))
    nnz = int(ptr[-1])
    for cap in (nnz - 1, 1):
        out_ptr, out_ec, out_cnt, n = np.full(9, -7, dtype=np.int32), np.full(nnz, -7, dtype=np.int32), np.full(nnz, -7, dtype=np.int32), C.c_uint64(99)
        rc = lib.ecb_resample(0, m.num_reads, 1, len(xn), ecb._ptr(pn), ecb._ptr(xn), ecb._ptr(dn), -1, 3, 0, 8, ecb._ptr(out_ptr), ecb._ptr(out_ec),
                              ecb._ptr(out_cnt), cap, C.byref(n))
        assert rc == 0 and n.value == nnz and np.array_equal(out_ptr, ptr) and (out_ec == -7).all() and (out_cnt == -7).all()
        d = [torch.as_tensor(a, device="cuda") for a in (pn, xn, dn, np.full(9, -7, dtype=np.int32), out_ec, out_cnt)]
        n = C.c_uint64(99)
        p = [C.c_void_p(t.data_ptr()) for t in d]
        rc = lib.ecb_resample_device(0, m.num_reads, 1, len(xn), p[0], p[1], p[2], -1, 3, 0, 8, p[3], p[4], p[5], cap, C.byref(n))
        torch.cuda.synchronize()
        assert rc == 0 and n.value == nnz and np.array_equal(d[3].cpu().numpy(), ptr) and (d[4].cpu().numpy() == -7).all() and (d[5].cpu().numpy() == -7).all()


# ---- the bootstrap --------------------------------------------------------------------------------------------------------------------------
B8, ITERS, TOL, SEED = 8, 40, 1e-5, 3


def _gene():
    m = load(C1)
    if "gene" not in _kept:
        _kept["gene"] = bin_utils.gene_ids(m, GRP)
    return _kept["gene"]


def _mats(m, tensors):
    a = [m.indptrA, m.indicesA, m.dataA, m.indptrN, m.indicesN, m.dataN]
    if tensors:
        a = [_dev(x, np.int32) for x in a]
    return a[0], a[1], a[2], m.num_loci, m.num_haplotypes, a[3], a[4], a[5]


def _boot(model=4, tensors=False, n_reps=B8, **kw):
    m = load(C1)
    if model != 4:
        gene, names = _gene()
        kw.update(gene=_dev(gene, np.int32) if tensors else gene, n_genes=len(names), model=model)
    kw.setdefault("max_iters", ITERS)
    kw.setdefault("tol", TOL)
    out = ecb_boot.quantify_bootstrap(*_mats(m, tensors), n_reps=n_reps, seed=SEED, return_reps=True, **kw)
    mean, sd, tm, ts, info, reps = out
    if tensors:
        assert all(t.is_cuda for t in (mean, sd, tm, ts, reps)) and all(info[k].is_cuda for k in INFO)
    return tuple(_np(t) for t in (mean, sd, tm, ts)) + ({k: _np(info[k]) for k in INFO}, _np(reps))


def _blob(res):
    mean, sd, tm, ts, info, reps = res
    return b"".join(np.ascontiguousarray(a).tobytes() for a in (mean, sd, tm, ts, reps)) + \
        b"".join(np.ascontiguousarray(info[k]).astype(np.float64).tobytes() for k in INFO)


def _kept_boot(model):
    if ("boot", model) not in _kept:
        _kept[("boot", model)] = _boot(model)
    return _kept[("boot", model)]


@pytest.mark.parametrize("model", [4, 2], ids=["flat", "M2"])
def test_the_bootstrap_is_quantify_cells_on_the_resampled_n_and_welford_over_it(model):
    m = load(C1)
    H, T = m.num_haplotypes, m.num_loci
    mean, sd, tm, ts, info, reps = _kept_boot(model)
    ptr, ec, cnt, _ = _golden(C1, None, B8)
    a = (m.indptrA, m.indicesA, m.dataA, T, H, ptr, ec, cnt)
    if model == 4:
        cp, sl, th, cinfo = ecb.quantify_cells(*a, max_iters=ITERS, tol=TOL)
    else:
        gene, names = _gene()
        cp, sl, th, cinfo = ecb.quantify_cells_model(*a, gene=gene, n_genes=len(names), model=model, max_iters=ITERS, tol=TOL)
    want = bc.scatter(cp, sl, th, T, H)
    assert reps.shape == (B8, H, T) and reps.tobytes() == want.tobytes()
    for k in INFO:
        assert np.array_equal(info[k], cinfo[k]), k
    assert len(set(info["n_iter"].tolist())) > 1 or info["n_iter"].max() == ITERS         # each replicate stops on its own
    # the moments: the checker's loop on these reps, within the bound of the docstring
    for got_m, got_s, x, what in ((mean, sd, reps, "entries"), (tm, ts, bc.totals(reps), "totals")):
        ref_m, ref_s, ref_M = bc.welford(x)
        X = np.abs(x).max(axis=0)
        bound_m, bound_M = 3 * B8 * EPS * X, ((7 * B8 + 3) * B8 + 3 * B8) * EPS * X * X
        dm, dM = np.abs(got_m - ref_m), np.abs(got_s ** 2 * (B8 - 1) - ref_M)
        live = X > 0
        print("model %d %s: worst |mean - ref| / bound %.3g, worst |M - ref| / bound %.3g" % (
            model, what, (dm[live] / bound_m[live]).max(), (dM[live] / bound_M[live]).max()))
        assert (dm <= bound_m).all() and (dM <= bound_M).all()
        # an entry that is 0 in every replicate: mean 0, sd 0
        assert (~live).any() and not got_m[~live].any() and not got_s[~live].any()
    assert (sd[reps.max(axis=0) > reps.min(axis=0)] > 0).all()


def test_one_replicate_is_its_own_mean_and_has_no_spread():
    mean, sd, tm, ts, info, reps = _boot(n_reps=1)
    assert mean.tobytes() == reps[0].tobytes() and not sd.any() and not ts.any()
    assert tm.tobytes() == bc.totals(reps)[0].tobytes()
    assert reps[0].tobytes() == _kept_boot(4)[5][0].tobytes()               # replicate 0 whatever the number of replicates


def _routes():
    """The flat and the model bootstrap by every route, as one blob each; asserts that the routes agree."""
    out = b""
    for model in (4, 2):
        first = _blob(_boot(model))
        for kw in ({"budget_bytes": 1}, {"tensors": True}, {"tensors": True, "budget_bytes": 1}, {}):
            assert _blob(_boot(model, **kw)) == first, (model, kw)
        out += first
    return out


def test_one_rule_for_every_route():
    first = _routes()
    assert first == _blob(_kept_boot(4)) + _blob(_kept_boot(2))
    _kept["digest"] = hashlib.sha256(first).hexdigest()


def test_everything_once_more_with_the_scratch_poisoned_gives_the_same_bits():
    if "digest" not in _kept:
        _kept["digest"] = hashlib.sha256(_routes()).hexdigest()
    env = dict(os.environ)
    env["ECB_POISON_SCRATCH"] = "1"
    env["ALNTOOLS_TORCH"] = "1"
    code = ("import sys, hashlib; sys.path[:0] = [%r, %r]; import test_gpu_ecboot as t; print('digest', hashlib.sha256(t._routes()).hexdigest())"
            % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "digest " + _kept["digest"] in r.stdout


def test_no_reads_or_no_alignments_is_no_error():
    m = load(C1)
    a = list(_mats(m, False))
    zero = a[:7] + [np.zeros_like(a[7])]
    for args in (zero, [np.zeros(m.num_reads + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)] + a[3:]):
        mean, sd, tm, ts, info, reps = ecb_boot.quantify_bootstrap(*args, n_reps=3, return_reps=True)
        assert not mean.any() and not sd.any() and not tm.any() and not ts.any() and not reps.any()
        assert info["converged"].all() and not info["n_iter"].any()


def _call(lib, m, over=None, tensors=False, **kw):
    """ecb_quantify_bootstrap on pre-filled outputs -> (rc, every output untouched)."""
    import torch
    H, T = m.num_haplotypes, m.num_loci
    v = dict(ip=m.indptrA, ix=m.indicesA, da=m.dataA, pn=m.indptrN, xn=m.indicesN, dn=m.dataN, scale=None, gene=None)
    v.update(over or {})
    p = dict(sample=-1, max_iters=5, tol=1e-6, budget=0, n_genes=0, model=4, seed=1, n_reps=2, n_ecs=m.num_reads, no_mean=False, no_sd=False)
    p.update(kw)
    B = max(p["n_reps"], 1)
    types = dict(ip=np.int32, ix=np.int32, da=np.int32, pn=np.int32, xn=np.int32, dn=np.int32, scale=np.float64, gene=np.int32)
    ins = {k: None if a is None else np.ascontiguousarray(a, dtype=types[k]) for k, a in v.items()}
    outs = [np.full(s, 7, dtype=dt) for s, dt in (((H, T), np.float64), ((H, T), np.float64), ((T,), np.float64), ((T,), np.float64), ((B, H, T), np.float64),
                                                  ((B,), np.uint32), ((B,), np.float64), ((B,), np.int64), ((B,), np.uint8))]
    if tensors:
        ins = {k: None if a is None else torch.as_tensor(a, device="cuda") for k, a in ins.items()}
        outs = [torch.as_tensor(o.view(np.int32) if o.dtype == np.uint32 else o, device="cuda") for o in outs]
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    else:
        ptr = ecb._ptr
    o = [ptr(x) for x in outs]
    if p["no_mean"]:
        o[0] = None
    if p["no_sd"]:
        o[1] = None
    fn = lib.ecb_quantify_bootstrap_device if tensors else lib.ecb_quantify_bootstrap
    rc = fn(0, p["n_ecs"], T, H, len(v["ix"]), ptr(ins["ip"]), ptr(ins["ix"]), ptr(ins["da"]), len(v["pn"]) - 1, len(v["xn"]), ptr(ins["pn"]), ptr(ins["xn"]),
            ptr(ins["dn"]), p["sample"], ptr(ins["scale"]), p["max_iters"], p["tol"], p["budget"], p["n_genes"], ptr(ins["gene"]), p["model"], p["seed"],
            p["n_reps"], *o)
    if tensors:
        torch.cuda.synchronize()
        outs = [x.cpu().numpy() for x in outs]
    return rc, all((x == 7).all() for x in outs)


def _refusals():
    m = load(C1)
    H, T = m.num_haplotypes, m.num_loci
    gene, names = _gene()
    bad_ix = m.indicesA.copy()
    bad_ix[5] = T
    neg = m.dataN.copy()
    neg[2] = -1
    nan = np.ones((H, T))
    nan[1, 3] = np.nan
    bad_gene = gene.copy()
    bad_gene[7] = len(names)
    huge = dict(pn=np.array([0, 2]), xn=np.array([0, 1]), dn=np.array([1 << 30, 1 << 30]))
    return [
        ("a-locus-beyond-T", dict(over=dict(ix=bad_ix)), CONTRACT), ("a-negative-count", dict(over=dict(dn=neg)), CONTRACT),
        ("an-unknown-sample", dict(sample=1), CONTRACT), ("a-nan-in-scale", dict(over=dict(scale=nan)), CONTRACT),
        ("a-gene-id-beyond-n_genes-M2", dict(over=dict(gene=bad_gene), n_genes=len(names), model=2), CONTRACT),
        ("a-gene-id-beyond-n_genes-M4", dict(over=dict(gene=bad_gene), n_genes=len(names), model=4), CONTRACT),
        ("model-5", dict(model=5), ARG), ("model-2-without-genes", dict(model=2), ARG), ("genes-without-n_genes", dict(over=dict(gene=gene), model=2), ARG),
        ("tol-nan", dict(tol=float("nan")), ARG), ("tol-negative", dict(tol=-1e-9), ARG), ("no-replicate", dict(n_reps=0), ARG),
        ("no-mean", dict(no_mean=True), ARG), ("no-sd", dict(no_sd=True), ARG), ("W-of-2^31", dict(over=huge), LIMIT),
    ]


REFUSED = ["a-locus-beyond-T", "a-negative-count", "an-unknown-sample", "a-nan-in-scale", "a-gene-id-beyond-n_genes-M2", "a-gene-id-beyond-n_genes-M4",
           "model-5", "model-2-without-genes", "genes-without-n_genes", "tol-nan", "tol-negative", "no-replicate", "no-mean", "no-sd", "W-of-2^31"]


@pytest.mark.parametrize("case", REFUSED)
def test_every_refusal_leaves_the_outputs_untouched(case):
    assert [r[0] for r in _refusals()] == REFUSED
    name, kw, code = next(r for r in _refusals() if r[0] == case)
    lib = ecb_boot.load()
    for tensors in (False, True):
        rc, untouched = _call(lib, load(C1), tensors=tensors, **kw)
        assert rc == code and untouched, (name, tensors, rc, lib.ecb_last_error(None))
    rc, untouched = _call(lib, load(C1))                               # ... and the same call without the fault runs
    assert rc == 0 and not untouched


def test_resample_refuses_replicate_numbers_beyond_32_bits_and_a_w_of_2_to_the_31():
    lib = ecb_boot.load()
    pn, xn, dn = np.array([0, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32), np.array([1 << 30, 1 << 30], dtype=np.int32)
    for b0, n_reps, data, sample, code in (((1 << 32) - 1, 2, [1, 1], -1, ARG), (1 << 32, 0, [1, 1], -1, ARG), (0, 1, [1 << 30, 1 << 30], -1, LIMIT),
                                            (0, 1, [1, -1], -1, CONTRACT), (0, 1, [1, 1], 1, CONTRACT)):
        dn = np.array(data, dtype=np.int32)
        out, n = np.full(4, -7, dtype=np.int32), C.c_uint64(99)
        rc = lib.ecb_resample(0, 2, 1, 2, ecb._ptr(pn), ecb._ptr(xn), ecb._ptr(dn), sample, 0, b0, n_reps, ecb._ptr(out), None, None, 0, C.byref(n))
        assert rc == code and (out == -7).all() and n.value == 99, (b0, n_reps, data, rc)
    out, n = np.full(2, -7, dtype=np.int32), C.c_uint64(99)
    dn = np.array([(1 << 30) - 1, 1 << 30], dtype=np.int32)                # W = 2^31 - 1 is counted, not drawn here: n_reps = 0
    assert lib.ecb_resample(0, 2, 1, 2, ecb._ptr(pn), ecb._ptr(xn), ecb._ptr(dn), -1, 0, 0, 0, ecb._ptr(out), None, None, 0, C.byref(n)) == 0 and n.value == 0


def test_the_command_end_to_end(tmp_path):
    m = load(C1)
    out, npy = str(tmp_path / "boot.tsv"), str(tmp_path / "reps.npy")
    env = dict(os.environ)
    env.pop("ALNTOOLS_GPUS", None)
    env["ALNTOOLS_TORCH"] = "0"
    r = subprocess.run([sys.executable, "-m", "alntools_amd.cli", "ecboot", C1, out, "-b", str(B8), "--seed", str(SEED), "-i", str(ITERS), "-t", str(TOL),
                        "--replicates", npy, "-v"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    mean, sd, tm, ts, info, reps = _kept_boot(4)
    theta = ecb.quantify(*_mats(m, False), max_iters=ITERS, tol=TOL)[0]
    assert open(out).read() == bin_utils.boot_table(m.lname, m.hname, theta, mean, sd, tm, ts)
    assert np.load(npy).tobytes() == reps.tobytes()
    r = subprocess.run([sys.executable, "-m", "alntools_amd.cli", "ecboot", C1, out + "2", "-b", "2", "-s", "NOPE"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 1 and "Error: sample NOPE is not in" in r.stderr and not os.path.exists(out + "2")
