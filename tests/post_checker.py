# -*- coding: utf-8 -*-
"""numpy restatement of ecquant's posterior (``include/ecb_quant_post.h``): one probability per set bit of A at a given theta for models 1-4, in
BIT ORDER (the non-zeros in storage order, the set bits of one lowest first); the permutation between bit order and EMASE's per-haplotype
CSC layout (``ecb_csr_to_hapcsc_values``); and the bounds.  float64 throughout.  Test infrastructure: the package has no CPU path for it.
``test_ecposterior.py`` pins it to the arrays recorded from the reference (``tests/golden/post_cases.json``).

The bounds are derived, not measured (the chains are spelled out in ``test_ecposterior.py``): relative, entry by entry, with exactly the same
entries 0 --

  model 4    (B + 4) 2^-52
  model 1    (B + R + 2 M H + 2 M + H + 6) 2^-52        each the bound of one step of that model (``quant_model_checker.Grouping.tolerance``)
  model 2    (R + 2 M H + M + 3 H + 6) 2^-52            without its L term: the posterior has no column sum
  model 3    (B + R + 2 M H + 5) 2^-52
"""
import json
import os

import numpy as np

import quant_checker as qchk
import quant_model_checker as mchk

GOLDEN = mchk.GOLDEN


def tolerance(model, B, H, M=0, R=0):
    """The relative bound of the posterior of ``model``, entry by entry."""
    n = {4: B + 4, 1: B + R + 2 * M * H + 2 * M + H + 6, 2: R + 2 * M * H + M + 3 * H + 6, 3: B + R + 2 * M * H + 5}[model]
    return n * 2.0 ** -52


class Layout(object):
    """Where the set bits of a CSR(bitmask) A sit in the three orders: bit order, ``quant_checker.Problem``'s (haplotype-major, the
    non-zeros in storage order within a haplotype) and EMASE's per-haplotype CSC (haplotype-major, columns ascending, rows ascending)."""

    def __init__(self, indptr, indices, data, n_loci, n_haps):
        indptr = np.asarray(indptr, dtype=np.int64)
        col = np.asarray(indices, dtype=np.int64)
        mask = np.asarray(data, dtype=np.int64)
        self.E, self.T, self.H, self.nnz = len(indptr) - 1, int(n_loci), int(n_haps), len(mask)
        row = np.repeat(np.arange(self.E), np.diff(indptr))
        pop = np.zeros(self.nnz, dtype=np.int64)
        for h in range(32):
            pop += (mask >> h) & 1
        self.bit_ptr = np.concatenate([[0], np.cumsum(pop)]).astype(np.int64)
        self.n_bits = int(self.bit_ptr[-1])
        hm, csc, cptr, cidx, self.bit_row = [], [], [], [], np.zeros(self.n_bits, dtype=np.int64)
        below = np.zeros(self.nnz, dtype=np.int64)                        # the set bits of each non-zero below haplotype h
        for h in range(self.H):
            has = np.flatnonzero((mask >> h) & 1)
            at = self.bit_ptr[has] + below[has]
            self.bit_row[at] = row[has]
            hm.append(at)
            order = np.argsort(col[has], kind="stable")                   # (rows ascend within a column: the CSR's rows do)
            csc.append(at[order])
            cidx.append(row[has][order])
            cptr.append(np.concatenate([[0], np.cumsum(np.bincount(col[has], minlength=self.T))]))
            below += (mask >> h) & 1
        cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)      # noqa: E731
        #: hm_to_bit[k] = the bit-order place of Problem's entry k; csc_to_bit[k] = that of the EMASE layout's entry k
        self.hm_to_bit, self.csc_to_bit = cat(hm), cat(csc)
        self.csc_indptr = np.array(cptr, dtype=np.int32).reshape(self.H, self.T + 1)
        self.csc_indices = cat(cidx).astype(np.int32)

    @classmethod
    def of(cls, m):
        return cls(m.indptrA, m.indicesA, m.dataA, m.num_loci, m.num_haplotypes)

    def to_csc(self, values):
        """values in bit order -> the EMASE layout (``csc_data``)."""
        return np.asarray(values)[self.csc_to_bit]

    def from_csc(self, csc_data):
        """The inverse of :meth:`to_csc`."""
        out = np.empty(self.n_bits, dtype=np.asarray(csc_data).dtype)
        out[self.csc_to_bit] = csc_data
        return out

    def hapcsc(self, values):
        """A ``hapcsc`` for ``emase_h5.save`` whose matrices carry ``values`` (bit order): what ``emase_h5.device_hapcsc_values`` must produce."""
        from alntools_amd import emase_h5
        data = self.to_csc(np.asarray(values, dtype=np.float64))
        return lambda m: emase_h5.split_hapcsc(self.csc_indptr, self.csc_indices, data)


def _ratio(num, den):
    out = np.zeros(len(num))
    np.divide(num, den, out=out, where=den > 0)
    return out


def posterior(q, lay, model, theta, scale=None):
    """(post in bit order, row_mass) of ``model`` over the grouping ``q`` (a ``quant_model_checker.Grouping``; for model 4 a
    ``quant_checker.Problem`` will do) of the matrix whose layout is ``lay``.  ``quant_model_checker.step`` without its weighted sum."""
    p = q if model == 4 and not hasattr(q, "p") else q.p
    H, T = p.H, p.T
    phi = np.asarray(theta, dtype=np.float64).reshape(-1)
    if scale is not None:
        phi = phi * np.asarray(scale, dtype=np.float64).reshape(-1)
    v = phi[p.bit_flat]
    row = p.bit_row
    d_row = np.bincount(row, weights=v, minlength=p.E) if p.E else np.zeros(0)
    if model == 4:
        post = _ratio(v, d_row[row])
    else:
        assert model in (1, 2, 3)
        G = q.G
        phi2 = phi.reshape(H, T)
        phi_gh = np.stack([np.bincount(q.gene, weights=phi2[h], minlength=G) for h in range(H)], axis=1) if T else np.zeros((G, H))
        phi_g = phi_gh.sum(axis=1)
        phi_t = phi2.sum(axis=0)
        seg, g = q.bit_seg, q.bit_g
        d_seg = mchk._group_sum(seg, v, q.n_seg)
        gd = mchk._group_sum(q.seg_row, phi_g[q.seg_gene], p.E, d_seg > 0)
        post = _ratio(phi_g[g], gd[row])
        if model == 3:
            post = post * _ratio(v, d_seg[seg])
        elif model == 1:
            key, sh = np.unique(seg * H + q.bit_h, return_inverse=True)
            d_sh = mchk._group_sum(sh, v, len(key))
            ad = mchk._group_sum(key // H, phi_gh[q.seg_gene[key // H], key % H], q.n_seg, d_sh > 0)
            post = post * _ratio(phi_gh[g, q.bit_h], ad[seg]) * _ratio(v, d_sh[sh])
        else:
            key, st = np.unique(seg * max(T, 1) + q.bit_t, return_inverse=True)
            d_t = mchk._group_sum(st, v, len(key))
            idn = mchk._group_sum(key // max(T, 1), phi_t[key % max(T, 1)], q.n_seg, d_t > 0)
            post = post * _ratio(phi_t[q.bit_t], idn[seg]) * _ratio(v, d_t[st])
        post = np.where(d_seg[seg] > 0, post, 0.0)
    out = np.zeros(lay.n_bits)
    out[lay.hm_to_bit] = post
    return out, d_row


def weighted_sum(p, lay, post):
    """theta'[h, t] = the sum over rows of w[e] times the posterior (``post`` in bit order): one step of the EM."""
    hm = np.asarray(post)[lay.hm_to_bit]
    return np.bincount(p.bit_flat, weights=p.w[p.bit_row].astype(np.float64) * hm, minlength=p.H * p.T).reshape(p.H, p.T)


# ---- the recorded cases (tests/golden/post_cases.json), shared by the CPU and GPU tests ----
CASES = json.load(open(os.path.join(GOLDEN, "post_cases.json")))["cases"]
TRIPLES = [(c, model, k) for c in CASES for model in c["models"] for k in c["steps"]]
TRIPLE_IDS = ["%s-m%d-k%d" % (c["name"], model, k) for c, model, k in TRIPLES]
_loaded = {}


class Recorded(object):
    """One recorded case: the matrices, the checker's problem and grouping, the layout, the thetas and the reference's arrays."""

    def __init__(self, case):
        from alntools_amd import bin_utils
        self.case = case
        self.m = bin_utils.ecload(os.path.join(GOLDEN, case["ec"]))
        self.p = qchk.Problem.of(self.m, None)
        self.lay = Layout.of(self.m)
        flat = np.load(os.path.join(GOLDEN, case["theta_flat"]))
        self.scale = flat["scale"] if case["use_lengths"] else None
        self.next = {(4, k): flat["next_%d" % k] for k in case["steps"]}
        self.theta = {(4, k): flat["theta_%d" % k] for k in case["steps"]}
        self.gene, self.G, self.q = None, 0, self.p
        if case["grp"] is not None:
            self.gene, self.G = mchk.genes_of(self.m, os.path.join(GOLDEN, case["grp"]))
            self.q = mchk.Grouping(self.p, self.gene, self.G)
            for model in (1, 2, 3):
                z = dict(np.load(os.path.join(GOLDEN, case["theta_model"] + ".npz")))
                for c in "ab":
                    z.update(np.load(os.path.join(GOLDEN, "%s_m%d_%s.npz" % (case["theta_model"], model, c))))
                for k in case["steps"]:
                    self.theta[(model, k)], self.next[(model, k)] = z["theta_%d" % k], z["theta_%d" % (k + 1)]
        z = {}
        for f in case["npz"]:
            z.update(np.load(os.path.join(GOLDEN, f)))
        self.rows = z.get("rows")
        #: which entries of the EMASE layout the case records (all, or those of ``rows``)
        self.kept = np.ones(self.lay.n_bits, dtype=bool) if self.rows is None else np.isin(self.lay.csc_indices, self.rows)
        self.ref = {}
        for model in case["models"]:
            for k in case["steps"]:
                key = "m%d_k%d" % (model, k)
                if key in z:
                    self.ref[(model, k)] = z[key]
                else:
                    n = len([x for x in z if x.startswith(key + "_p")])
                    self.ref[(model, k)] = np.concatenate([z["%s_p%d" % (key, i)] for i in range(n)])

    def grouping(self, model):
        return self.p if model == 4 else self.q

    def bound(self, model):
        c = self.case
        return tolerance(model, c["B"], self.p.H, c["M"], c["R"])

    def step_bound(self, model):
        """The bound of one whole step of ``model``: the ``Σ w p = theta'`` checks use it unchanged."""
        return self.p.tolerance() if model == 4 else self.q.tolerance(model)

    def recorded_of(self, post):
        """The entries of ``post`` (bit order) the case records, in the recorded order."""
        return self.lay.to_csc(post)[self.kept]


def load_case(case):
    if case["name"] not in _loaded:
        _loaded[case["name"]] = Recorded(case)
    return _loaded[case["name"]]
