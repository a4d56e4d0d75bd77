#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""Generate the fixtures of ecquant's posterior (``post_*``) in this directory by RUNNING THE REFERENCE.

Build-container only, like ``make_golden_quant_models.py``, whose ``Case`` it imports: the unmodified reference package from
``/root/reference`` with the stand-ins of ``_standins/`` ahead of it.  What is recorded is what the reference's calls leave in the matrix
BEFORE its weighted sum over reads, at the theta_0 and theta_5 the existing ``quant_<case>.npz`` / ``quant_model_<case>*.npz`` hold:

  flat model (4)   ``reset(); multiply(phi, axis=2); normalize_reads(axis=READ)``: every haplotype's data at its aligned entries
  models 1-3       the ``post`` arrays ``Case.step`` forms -- the product of the reference's own factors -- before ``sum(axis=READ)``

each as ONE array in EMASE's layout: haplotype 0's aligned entries in csc order (columns ascending, rows ascending within one), then
haplotype 1's, ...; a 0/0 (a row none of whose targets has any abundance) read as 0.  As ``make_golden_quant_models.py`` does, the script
asserts that no recorded theta puts any row under the deviation (a gene, allele or isoform with D = 0 and Phi > 0).  Records data only:

  post_cases.json            every case: the .bin, the group file, whether scale = 1 / length, the shape, the models and steps k recorded, B, L,
                             M, R (as ``quant_model_cases.json`` defines them; M = R = 0 for a case with the flat model alone), where theta
                             comes from, and the .npz files
  post_<case>_<a|b|...>.npz  ``m<model>_k<k>`` (float64), cut into pieces ``m<model>_k<k>_p<i>`` where one array does not fit a file: each
                             file stays within LIMIT.  The first file also holds ``rows`` (int64, ascending) when the case records a subset
                             of the rows only: the entries of the other rows are left out of every array.

``h8`` has one row of 3 598 set bits and ~0.9 M aligned entries: it records that row, the 200 rows after it and every 10th row.

    python tests/golden/make_golden_post.py
"""
from __future__ import print_function

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

from make_golden_quant_models import Case, partition, at, bin_utils  # noqa: E402  (puts the reference and the stand-ins on the path)

# name, .bin, source group file (None: the flat model alone), scale = 1 / length, records a subset of the rows
CASES = [("c1", "g2_c1.bin", "gt_c1.grp.txt", False, False), ("ms", "g4b_multi_min0.bin", "gt_ms.grp.txt", False, False),
         ("c1_len", "g2_c1.bin", None, True, False), ("h8", "gt_h8_in.bin", "gt_h8.grp.txt", False, True)]
STEPS = (0, 5)
LIMIT = 970265          # bytes: no .npz larger than the largest fixture already here
PIECE = 118000          # float64 values to a file: 944 000 bytes before compression, so a file fits whatever its values are


class PostCase(Case):
    def posts(self, model, theta, scale):
        """The ``post`` arrays of ``Case.step``, per haplotype in csc order: the matrix it fills before ``sum(axis=READ)``, which copies.
        ``Case.step`` hands out its result alone, so the matrix is caught where it is made (the last ``base.copy()`` without arguments) and
        the catch is checked: the caught matrix's own weighted sum must be the theta' the step returned, bit for bit, and its count w."""
        real, made = self.base, []

        class Spy(object):
            def __getattr__(self, name):
                return getattr(real, name)

            def copy(self, *a, **k):
                out = real.copy(*a, **k)
                if not a and not k:
                    made.append(out)
                return out
        self.base = Spy()
        try:
            nxt = Case.step(self, model, theta, scale)
        finally:
            self.base = real
        out = made[-1]
        assert np.array_equal(out.count, self.w.astype(np.float64))
        assert np.asarray(out.sum(axis=out.Axis.READ), dtype=np.float64).tobytes() == np.asarray(nxt, dtype=np.float64).tobytes()
        for h in range(self.H):                              # (and it has the incidence's own structure: the values are in csc order)
            assert np.array_equal(out.data[h].indices, self.coords[h][0]) and len(out.data[h].data) == len(self.coords[h][0])
        return [np.array(out.data[h].data, dtype=np.float64) for h in range(self.H)]

    def flat(self, theta, scale):
        phi = theta if scale is None else theta * scale
        m = self.apm.copy()
        m.reset()
        m.multiply(phi, axis=2)
        with np.errstate(divide="ignore", invalid="ignore"):
            m.normalize_reads(axis=m.Axis.READ)
        out = []
        for h in range(self.H):
            v = np.array(at(m.data[h], *self.coords[h]), dtype=np.float64)
            v[~np.isfinite(v)] = 0.0
            out.append(v)
        return out


def main():
    cases = []
    for name, ec, grp, use_len, subset in CASES:
        apm = bin_utils.ecload(os.path.join(HERE, ec))
        T, H, E = (int(x) for x in apm.shape)
        flat_z = np.load(os.path.join(HERE, "quant_%s.npz" % name))
        w = flat_z["w"]
        scale = flat_z["scale"] if use_len else None
        if grp is not None:
            gene, names, groups = partition(apm, os.path.join(HERE, grp), os.devnull)
            model_z = np.load(os.path.join(HERE, "quant_model_%s.npz" % name))
            assert np.array_equal(gene, model_z["gene"]) and np.array_equal(w, model_z["w"])
        else:
            gene, names, groups = np.arange(T, dtype=np.int32), list(apm.lname), [[t] for t in range(T)]
        k = PostCase(apm, w, gene, names, groups)
        models = [4] + ([1, 2, 3] if grp is not None else [])
        keep = None
        rows = None
        if subset:
            bits = np.zeros(E, dtype=np.int64)
            for r, _ in k.coords:
                bits += np.bincount(r, minlength=E)
            big = int(np.argmax(bits))
            rows = np.unique(np.concatenate([np.arange(big, min(E, big + 201)), np.arange(0, E, 10)]))
            keep = np.concatenate([np.isin(r, rows) for r, _ in k.coords])
        arrays = {}
        for model in models:
            for s in STEPS:
                if model == 4:
                    theta = flat_z["theta_%d" % s]
                    post = k.flat(theta, scale)
                else:
                    theta = None
                    for f in ["quant_model_%s.npz" % name] + ["quant_model_%s_m%d_%s.npz" % (name, model, c) for c in "ab"]:
                        z = np.load(os.path.join(HERE, f))
                        if "theta_%d" % s in z:
                            theta = z["theta_%d" % s]
                    assert theta is not None and theta.shape == (H, T)
                    assert not k.deviating(theta if scale is None else theta * scale), (name, model, s)
                    post = k.posts(model, theta, scale)
                post = np.concatenate(post)
                assert post.shape == (sum(len(r) for r, _ in k.coords),) and np.all(np.isfinite(post)) and np.all(post >= 0) and np.all(post <= 1.0 + 1e-9)
                arrays["m%d_k%d" % (model, s)] = post if keep is None else post[keep]
        # files: the arrays in order, cut so that no file holds more than PIECE values
        files, cur, room = [], {}, PIECE
        if rows is not None:
            cur["rows"] = rows.astype(np.int64)
        for key in sorted(arrays):
            a, i, whole = arrays[key], 0, len(arrays[key]) <= room
            if whole:
                cur[key] = a
                room -= len(a)
                continue
            at0 = 0
            while at0 < len(a) or (len(a) == 0 and i == 0):
                if room == 0:
                    files.append(cur)
                    cur, room = {}, PIECE
                n = min(room, len(a) - at0)
                cur["%s_p%d" % (key, i)] = a[at0:at0 + n]
                at0, i, room = at0 + n, i + 1, room - n
                if len(a) == 0:
                    break
        if cur:
            files.append(cur)
        fnames = ["post_%s_%s.npz" % (name, "abcdefghijklmnopqrstuvwxyz"[i]) for i in range(len(files))]
        sizes = []
        for fname, what in zip(fnames, files):
            path = os.path.join(HERE, fname)
            np.savez_compressed(path, **what)
            assert os.path.getsize(path) <= LIMIT, (fname, os.path.getsize(path))
            sizes.append(os.path.getsize(path))
        bits = np.zeros(E, dtype=np.int64)
        L = 0
        for h in range(H):
            d = k.base.data[h].tocsc()
            bits += np.bincount(d.indices, minlength=E)
            L = max(L, int(np.diff(d.indptr).max()))
        M = R = 0
        if grp is not None:
            seg = np.unique(np.concatenate([r.astype(np.int64) * k.G + gene[c] for r, c in k.coords]))
            M, R = int(np.bincount(gene).max()), int(np.bincount(seg // k.G).max())
        case = {"name": name, "ec": ec, "grp": None if grp is None else "quant_model_%s.grp.txt" % name, "use_lengths": use_len, "shape": [T, H, E],
                "models": models, "steps": list(STEPS), "B": int(bits.max()), "L": L, "M": M, "R": R, "subset": bool(subset),
                "theta_flat": "quant_%s.npz" % name, "theta_model": None if grp is None else "quant_model_%s" % name, "npz": fnames}
        cases.append(case)
        print(name, case["shape"], "B", case["B"], "L", L, "M", M, "R", R, "entries", len(next(iter(arrays.values()))), sizes, "bytes")
    with open(os.path.join(HERE, "post_cases.json"), "w") as f:          # (one case per line)
        f.write('{"cases":[\n%s\n]}\n' % ",\n".join(json.dumps(c, separators=(",", ":"), sort_keys=True) for c in cases))


if __name__ == "__main__":
    main()
