# -*- coding: utf-8 -*-
"""numpy restatement of ecquant's hierarchical models (``include/ecb_quant_model.h``): one EM step of model 1 (gene -> allele -> isoform),
2 (gene -> isoform -> allele) or 3 (gene -> isoform x allele) over a gene grouping, every normalizing sum over the members whose own D is
positive only; model 4 is ``quant_checker.step`` itself.  float64 throughout, one entry per set bit (``quant_checker.Problem``).  Test
infrastructure: the package has no CPU path for it.  ``test_ecquant_models.py`` pins it to the step pairs recorded from the reference's own
factors (``tests/golden/quant_model_cases.json``).

``reference_rule=True`` restates the reference's denominators instead -- a gene, allele or isoform the row touches stays in the sum
whatever its D -- to show, on hand-built rows, where that rule loses mass."""
import numpy as np

import quant_checker as qchk


class Grouping(object):
    """A :class:`quant_checker.Problem` with ``gene[t]``: the segments (row, gene) of the set bits and the lengths of the model's sums."""

    def __init__(self, p, gene, n_genes):
        gene = np.asarray(gene, dtype=np.int64)
        assert gene.shape == (p.T,) and (p.T == 0 or (gene.min() >= 0 and gene.max() < n_genes))
        self.p, self.gene, self.G = p, gene, int(n_genes)
        self.bit_t = p.bit_flat % max(p.T, 1)
        self.bit_h = p.bit_flat // max(p.T, 1)
        self.bit_g = gene[self.bit_t] if len(self.bit_t) else np.zeros(0, dtype=np.int64)
        # segments: the (row, gene) pairs that hold a set bit
        seg_key, self.bit_seg = np.unique(p.bit_row * max(self.G, 1) + self.bit_g, return_inverse=True)
        self.seg_row, self.seg_gene = seg_key // max(self.G, 1), seg_key % max(self.G, 1)
        self.n_seg = len(seg_key)
        #: M = the most members of a gene, R = the most genes in a row
        self.M = int(np.bincount(gene, minlength=max(self.G, 1)).max()) if p.T else 0
        self.R = int(np.bincount(self.seg_row, minlength=max(p.E, 1)).max()) if p.E else 0

    def tolerance(self, model):
        """The relative bound of one step, entry by entry (derived in ``test_ecquant_models.py``)."""
        B, L, H, M, R = self.p.B, self.p.L, self.p.H, self.M, self.R
        if model == 4:
            return self.p.tolerance()
        n = {1: B + L + R + 2 * M * H + 2 * M + H + 6, 2: L + R + 2 * M * H + M + 3 * H + 6, 3: B + L + R + 2 * M * H + 5}[model]
        return n * 2.0 ** -52


def _group_sum(index, weights, n, only=None):
    if only is not None:
        index, weights = index[only], weights[only]
    return np.bincount(index, weights=weights, minlength=n) if n else np.zeros(0)


def _ratio(num, den):
    out = np.zeros(len(num))
    np.divide(num, den, out=out, where=den > 0)
    return out


def step(q, model, theta, scale=None, reference_rule=False):
    """(theta', explained) of one step of ``model`` over the grouping ``q``."""
    p = q.p
    if model == 4:
        return qchk.step(p, theta, scale)
    assert model in (1, 2, 3)
    H, T, G = p.H, p.T, q.G
    phi = np.asarray(theta, dtype=np.float64).reshape(-1)
    if scale is not None:
        phi = phi * np.asarray(scale, dtype=np.float64).reshape(-1)
    phi2 = phi.reshape(H, T)
    phi_gh = np.stack([np.bincount(q.gene, weights=phi2[h], minlength=G) for h in range(H)], axis=1) if T else np.zeros((G, H))   # G x H
    phi_g = phi_gh.sum(axis=1)
    phi_t = phi2.sum(axis=0)
    v = phi[p.bit_flat]                                               # phi of every set bit
    seg, row, g = q.bit_seg, p.bit_row, q.bit_g
    d_seg = _group_sum(seg, v, q.n_seg)
    seg_in = (d_seg > 0) | reference_rule                             # the genes of a row that count in its gene denominator
    gd = _group_sum(q.seg_row, phi_g[q.seg_gene], p.E, seg_in)
    d_row = _group_sum(row, v, p.E)
    post = _ratio(phi_g[g], gd[row])                                  # the gene factor
    if model == 3:
        post = post * _ratio(v, d_seg[seg])
    elif model == 1:
        key, sh = np.unique(seg * H + q.bit_h, return_inverse=True)   # (segment, haplotype)
        d_sh = _group_sum(sh, v, len(key))
        sh_in = (d_sh > 0) | reference_rule
        ad = _group_sum(key // H, phi_gh[q.seg_gene[key // H], key % H], q.n_seg, sh_in)
        post = post * _ratio(phi_gh[g, q.bit_h], ad[seg]) * _ratio(v, d_sh[sh])
    else:
        key, st = np.unique(seg * max(T, 1) + q.bit_t, return_inverse=True)   # (segment, target): a non-zero
        d_t = _group_sum(st, v, len(key))
        t_in = (d_t > 0) | reference_rule
        idn = _group_sum(key // max(T, 1), phi_t[key % max(T, 1)], q.n_seg, t_in)
        post = post * _ratio(phi_t[q.bit_t], idn[seg]) * _ratio(v, d_t[st])
    post = np.where(d_seg[seg] > 0, post, 0.0)
    new = np.bincount(p.bit_flat, weights=p.w[row].astype(np.float64) * post, minlength=H * T)
    return new.reshape(H, T), int(p.w[d_row > 0].sum())


def run(q, model, scale=None, theta_in=None, max_iters=1000, tol=1e-6):
    """(theta, info) as ``ecb.quantify_model`` returns them."""
    p = q.p
    theta = p.aln() if theta_in is None else np.array(theta_in, dtype=np.float64).reshape(p.H, p.T)
    info = {"n_iter": 0, "delta": 0.0, "explained": 0, "converged": False}
    if p.E == 0 or p.nnz == 0:
        info["converged"] = True
        return np.zeros((p.H, p.T)), info
    stop = tol * float(p.W)
    while info["n_iter"] < max_iters:
        new, info["explained"] = step(q, model, theta, scale)
        info["delta"] = qchk.delta(new, theta)
        theta = new
        info["n_iter"] += 1
        if info["delta"] <= stop:
            info["converged"] = True
            break
    return theta, info


def genes_of(m, grp_filename):
    """(gene[t], G) of a group file over the targets of ``m``: ``bin_utils.gene_ids``."""
    from alntools_amd import bin_utils
    gene, names = bin_utils.gene_ids(m, grp_filename)
    return gene, len(names)


# ---- the recorded cases (tests/golden/quant_model_cases.json) and the hand-built rows of the deviation, shared by the CPU and GPU tests ----
import json  # noqa: E402
import os  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = json.load(open(os.path.join(GOLDEN, "quant_model_cases.json")))["cases"]
MODELS = (1, 2, 3)
TRIPLES = [(c, model, k) for c in CASES for model in c["models"] for k in c["steps"]]
TRIPLE_IDS = ["%s-m%d-k%d" % (c["name"], model, k) for c, model, k in TRIPLES]
_loaded = {}


def load_case(case):
    """(ECMatrices, Grouping, the recorded arrays, scale or None) of one recorded case, loaded once: ``z["theta_0"]`` and, per model m,
    ``z[m]["theta_<k>"]`` -- the pair of step k is ``pair(z, m, k)``."""
    if case["name"] not in _loaded:
        from alntools_amd import bin_utils
        m = bin_utils.ecload(os.path.join(GOLDEN, case["ec"]))
        z = dict(np.load(os.path.join(GOLDEN, case["npz"])))
        for model, files in case["npz_model"].items():
            z[int(model)] = {"theta_0": z["theta_0"]}
            for f in files:
                z[int(model)].update(np.load(os.path.join(GOLDEN, f)))
        gene, G = genes_of(m, os.path.join(GOLDEN, case["grp"]))
        _loaded[case["name"]] = (m, Grouping(qchk.Problem.of(m, case["sample"]), gene, G), z, z.get("scale"))
    return _loaded[case["name"]]


def pair(z, model, k):
    return z[model]["theta_%d" % k], z[model]["theta_%d" % (k + 1)]


def deviation_cases():
    """Three hand-built matrices of 3 rows (H = 2, gene A = {t0, t1}, gene B = {t2}) in which row 0 touches a member whose own D is 0 while
    its Phi is positive: -> [(name, the models it bears on, Problem, gene, G, theta)].  Row 0 weighs 10, rows 1 and 2 keep the other
    targets' abundances alive."""
    gene, G = np.array([0, 0, 1]), 2
    n = ([0, 3], [0, 1, 2], [10, 3, 5])
    out = []
    # a gene: row 0 touches A only at t0, whose abundance is 0, while A has abundance at t1; and B at t2
    p = qchk.Problem([0, 2, 3, 4], [0, 2, 1, 2], [3, 1, 3, 3], 3, 2, *n)
    out.append(("gene", (1, 2, 3), p, gene, G, np.array([[0.0, 4.0, 2.0], [0.0, 1.0, 3.0]])))
    # an allele: row 0 touches A at t0 with both bits; h0 has no abundance at t0 but has at t1
    p = qchk.Problem([0, 1, 2, 3], [0, 1, 2], [3, 3, 3], 3, 2, *n)
    out.append(("allele", (1,), p, gene, G, np.array([[0.0, 4.0, 2.0], [6.0, 1.0, 3.0]])))
    # an isoform: row 0 touches t0 at h0 alone, where it has no abundance while its h1 has; and t1
    p = qchk.Problem([0, 2, 3, 4], [0, 1, 1, 2], [1, 3, 3, 3], 3, 2, *n)
    out.append(("isoform", (2,), p, gene, G, np.array([[0.0, 4.0, 2.0], [6.0, 1.0, 3.0]])))
    return out
