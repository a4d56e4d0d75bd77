#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""Generate the fixtures of ecquant's hierarchical models (``quant_model_*``) in this directory by RUNNING THE REFERENCE.

Build-container only, like ``make_golden_quant.py``: imports the unmodified reference package from ``/root/reference`` with the stand-ins
of ``_standins/`` ahead of it.  One step of a model is the product of the reference's own factors on the aligned entries, then its weighted
sum over reads (``sum(axis=READ)`` with ``count = w``):

  the last factor      ``reset(); multiply(phi, axis=2); normalize_reads(axis=HAPLOGROUP | LOCUS | GROUP, grouping_mat)`` for model 1 | 2 | 3,
                       ``grouping_mat`` the T x T same-gene incidence
  model 1's allele     ``bundle(reset=True)``, then ``multiply(Phi_GH, axis=2); normalize_reads(axis=LOCUS)``
  the gene factor      the bundle summed over haplotypes as a one-haplotype matrix, ``reset(); multiply(Phi_G, axis=2);
                       normalize_reads(axis=READ)``
  model 2's isoform    the matrix summed over haplotypes as a one-haplotype matrix, ``reset(); multiply(Phi_T, axis=2);
                       normalize_reads(axis=GROUP, grouping_mat)``

(the reference takes the one-haplotype matrices: no factor is computed here).  ``normalize_reads`` returns dense matrices whose entries
outside the incidence are NaN or infinite; only the aligned entries are read.  Phi_GH, Phi_G and Phi_T, the multipliers, are sums of phi
taken here with numpy.  Records data only:

  quant_model_cases.json       every case: the .bin, the group file, the sample, whether scale = 1 / length, the shape, G, the steps k, B, L,
                               M (the most members of a gene), R (the most genes in a row) and the .npz
  quant_model_<case>.grp.txt   the partition the case uses: of the source group file every target under the first group that lists it, a
                               group left without members dropped; the targets on no line are genes of their own
  quant_model_<case>.npz       ``w``, ``gene`` (T, int32: genes in file order, then the unlisted targets in target order), ``scale`` when the
                               case has one, and ``theta_0`` = aln (H x T float64), where every model's run starts
  quant_model_<case>_m<m>_<a|b|...>.npz   model m's own run from theta_0: ``theta_<k>`` and ``theta_<k+1>`` (H x T float64) for every
                               recorded k -- the pair of step k is (theta_k, theta_{k+1}) -- two arrays to a file, which keeps each within LIMIT

The recorded pairs are the ones where the reference's rule and ecquant's are the same: the script asserts that in no recorded pair any row
has a gene, allele or isoform with D = 0 and Phi > 0 (the share of rows under the deviation is 0), and that every recorded value is finite.

    python tests/golden/make_golden_quant_models.py
"""
from __future__ import print_function

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.join(HERE, "_standins"))

import numpy as np  # noqa: E402
from scipy.sparse import csc_matrix  # noqa: E402

from alntools import bin_utils  # noqa: E402  (the reference)

# name, .bin, source group file, sample column (None = pooled), scale = 1 / length
CASES = [("c1", "g2_c1.bin", "gt_c1.grp.txt", None, False), ("h8", "gt_h8_in.bin", "gt_h8.grp.txt", None, False),
         ("ms", "g4b_multi_min0.bin", "gt_ms.grp.txt", None, False), ("c1_len", "g2_c1.bin", "gt_c1.grp.txt", None, True)]
STEPS = (0, 1, 5)
MODELS = (1, 2, 3)
LIMIT = 970265          # bytes: no .npz larger than the largest fixture already here


def partition(apm, src, dst):
    """The partition ``src`` induces (first listing wins), written to ``dst``; returns (gene[t], gene names, per gene its targets)."""
    lid = dict(zip(apm.lname, range(len(apm.lname))))
    gene = np.full(len(apm.lname), -1, dtype=np.int32)
    names, lines = [], []
    with open(src) as fh:
        for line in fh:
            item = line.rstrip().split("\t")
            mine = []
            for t in item[1:]:
                if gene[lid[t]] < 0:
                    gene[lid[t]] = len(names)
                    mine.append(t)
            if mine:
                names.append(item[0])
                lines.append("\t".join([item[0]] + mine))
    with open(dst, "w") as fh:
        fh.write("".join(ln + "\n" for ln in lines))
    for t in np.flatnonzero(gene < 0):
        gene[t] = len(names)
        names.append(apm.lname[t])
    return gene, names, [np.flatnonzero(gene == g).tolist() for g in range(len(names))]


def one_hap(like, mat):
    """A one-haplotype matrix of the reference's own class around ``mat`` (reads x loci)."""
    m = like.copy(shallow=True)
    m.data = [csc_matrix(mat)]
    m.shape = (mat.shape[1], 1, mat.shape[0])
    m.num_loci, m.num_haplotypes, m.num_reads = m.shape
    m.reset()
    return m


def at(mat, rows, cols):
    """The entries (rows, cols) of what normalize_reads left: a dense matrix, or a sparse one."""
    if hasattr(mat, "tocsr"):
        return np.asarray(mat.tocsr()[rows, cols]).ravel()
    return np.asarray(mat)[rows, cols]


class Case(object):
    def __init__(self, apm, w, gene, names, groups):
        self.apm, self.w, self.gene = apm, w, gene
        self.T, self.H, self.E = (int(x) for x in apm.shape)
        self.G = len(names)
        apm.groups, apm.gname, apm.num_groups = groups, np.array(names), self.G
        self.base = apm.copy()
        self.base.reset()
        self.coords = []                                      # per haplotype: (rows, cols) of its aligned entries, in csc order
        for h in range(self.H):
            d = self.base.data[h]
            assert not (d.data == 0).any()
            self.coords.append((d.indices.copy(), np.repeat(np.arange(self.T), np.diff(d.indptr))))
        self.same_gene = csc_matrix((gene[:, None] == gene[None, :]).astype(np.float64))
        self.conv = np.zeros((self.T, self.G))
        self.conv[np.arange(self.T), gene] = 1.0
        self.bundle = self.base.bundle(reset=True)            # reads x genes per haplotype
        self.bundle.lengths = np.zeros((self.G, self.H))      # (bundle() leaves none, and copy() wants one)
        self.bundle_any =self.bundle.sum(axis=self.bundle.Axis.HAPLOTYPE)
        self.any = self.base.sum(axis=self.base.Axis.HAPLOTYPE)

    def theta0(self):
        m = self.base.copy()
        m.count = self.w.astype(np.float64)
        return np.asarray(m.sum(axis=m.Axis.READ), dtype=np.float64)

    def deviating(self, phi):
        """Does any row hold a gene, allele or isoform with D = 0 and Phi > 0?"""
        phi_gh = phi.dot(self.conv)                           # H x G
        phi_g, phi_t = phi_gh.sum(axis=0), phi.sum(axis=0)
        row = np.concatenate([r for r, _ in self.coords])
        col = np.concatenate([c for _, c in self.coords])
        hap = np.concatenate([np.full(len(r), h) for h, (r, _) in enumerate(self.coords)])
        v = phi[hap, col]
        g = self.gene[col]

        def lost(key, big):
            k, inv = np.unique(key, return_inverse=True)
            d = np.bincount(inv, weights=v, minlength=len(k))
            return bool(((d == 0) & (big[np.unique(inv, return_index=True)[1]] > 0)).any())
        seg = row.astype(np.int64) * self.G + g
        return lost(seg, phi_g[g]) or lost(seg * self.H + hap, phi_gh[hap, g]) or lost(row.astype(np.int64) * self.T + col, phi_t[col])

    def step(self, model, theta, scale):
        phi = theta if scale is None else theta * scale
        A = self.apm.Axis
        with np.errstate(divide="ignore", invalid="ignore"):
            m = self.apm.copy()
            m.reset()
            m.multiply(phi, axis=2)
            m.normalize_reads(axis={1: A.HAPLOGROUP, 2: A.LOCUS, 3: A.GROUP}[model], grouping_mat=self.same_gene)
            last = [at(m.data[h], *self.coords[h]) for h in range(self.H)]
            phi_gh = phi.dot(self.conv)
            gf = one_hap(self.bundle, self.bundle_any)
            gf.multiply(phi_gh.sum(axis=0, keepdims=True), axis=2)
            gf.normalize_reads(axis=A.READ)
            gene_f = gf.data[0]
            mid = None
            if model == 1:
                b = self.bundle.copy()
                b.multiply(phi_gh, axis=2)
                b.normalize_reads(axis=A.LOCUS)
                mid = [at(b.data[h], self.coords[h][0], self.gene[self.coords[h][1]]) for h in range(self.H)]
            elif model == 2:
                iso = one_hap(self.base, self.any)
                iso.multiply(phi.sum(axis=0, keepdims=True), axis=2)
                iso.normalize_reads(axis=A.GROUP, grouping_mat=self.same_gene)
                mid = [at(iso.data[0], *self.coords[h]) for h in range(self.H)]
            out = self.base.copy()
            for h in range(self.H):
                rows, cols = self.coords[h]
                post = at(gene_f, rows, self.gene[cols]) * last[h]
                if mid is not None:
                    post = post * mid[h]
                post[~np.isfinite(post)] = 0.0            # 0/0: an entry none of whose row's targets has any abundance, read as 0
                out.data[h].data = post
            out.count = self.w.astype(np.float64)
            return np.asarray(out.sum(axis=A.READ), dtype=np.float64)


def main():
    cases = []
    for name, ec, grp, sample, use_len in CASES:
        apm = bin_utils.ecload(os.path.join(HERE, ec))
        T, H, E = (int(x) for x in apm.shape)
        if type(apm.count) == csc_matrix:
            c = apm.count.tocsc()
            w = np.asarray(c.sum(axis=1)).ravel() if sample is None else np.asarray(c[:, sample].todense()).ravel()
        else:
            assert sample is None
            w = np.asarray(apm.count).ravel()
        assert w.shape == (E,) and np.all(w == np.round(w)) and np.all(w >= 0)
        w = w.astype(np.int64)
        grp_out = "quant_model_%s.grp.txt" % name
        gene, names, groups = partition(apm, os.path.join(HERE, grp), os.path.join(HERE, grp_out))
        members = np.bincount(gene)
        if name == "c1":
            assert (len(names), int(members.max()), int((members > 1).sum())) == (401, 5, 236), (len(names), members.max(), (members > 1).sum())
        k = Case(apm, w, gene, names, groups)
        theta0 = k.theta0()
        assert theta0.shape == (H, T)
        arrays = {"w": w, "gene": gene}
        scale = None
        if use_len:
            lens = np.asarray(apm.lengths, dtype=np.float64).T[:H]
            assert lens.shape == (H, T) and np.all(lens[theta0 > 0] > 0)
            scale = np.zeros((H, T))
            np.divide(1.0, lens, out=scale, where=lens > 0)
            arrays["scale"] = scale
        arrays["theta_0"] = theta0
        per_model = {}
        for model in MODELS:
            theta = theta0
            mine = per_model[model] = {}
            for s in range(max(STEPS) + 1):
                nxt = k.step(model, theta, scale)
                if s in STEPS:
                    assert not k.deviating(theta if scale is None else theta * scale), (name, model, s)
                    mine["theta_%d" % s], mine["theta_%d" % (s + 1)] = theta, nxt
                    for a in (theta, nxt):
                        assert np.all(np.isfinite(a)) and np.all(a >= 0)
                theta = nxt
        bits = np.zeros(E, dtype=np.int64)
        L = 0
        for h in range(H):
            d = k.base.data[h].tocsc()
            bits += np.bincount(d.indices, minlength=E)
            L = max(L, int(np.diff(d.indptr).max()))
        seg = np.unique(np.concatenate([r.astype(np.int64) * k.G + gene[c] for r, c in k.coords]))
        case = {"name": name, "ec": ec, "grp": grp_out, "sample": sample, "use_lengths": use_len, "shape": [T, H, E], "G": k.G, "steps": list(STEPS),
                "models": list(MODELS), "B": int(bits.max()), "L": L, "M": int(members.max()), "R": int(np.bincount(seg // k.G).max()),
                "npz": "quant_model_%s.npz" % name, "npz_model": {}}
        files = [(case["npz"], arrays)]
        for m in MODELS:
            keys = sorted((key for key in per_model[m] if key != "theta_0"), key=lambda key: int(key.split("_")[1]))
            chunks = [keys[i:i + 2] for i in range(0, len(keys), 2)]
            case["npz_model"][str(m)] = ["quant_model_%s_m%d_%s.npz" % (name, m, "abcdefgh"[i]) for i in range(len(chunks))]
            files += [(f, {key: per_model[m][key] for key in ch}) for f, ch in zip(case["npz_model"][str(m)], chunks)]
        sizes = []
        for fname, what in files:
            path = os.path.join(HERE, fname)
            np.savez_compressed(path, **what)
            assert os.path.getsize(path) <= LIMIT, (fname, os.path.getsize(path))
            sizes.append(os.path.getsize(path))
        cases.append(case)
        print(name, case["shape"], "G", k.G, "B", case["B"], "L", L, "M", case["M"], "R", case["R"], sizes, "bytes")
    with open(os.path.join(HERE, "quant_model_cases.json"), "w") as f:          # (one case per line)
        f.write('{"cases":[\n%s\n]}\n' % ",\n".join(json.dumps(c, separators=(",", ":"), sort_keys=True) for c in cases))


if __name__ == "__main__":
    main()
