#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""Search for true collisions of the EC table's 64-bit set hash and write them to ``hash_collisions.json`` in this directory.

Our own code: the hash is ``tests/set_hash.py`` (numpy), nothing is imported from the reference and nothing from the library.  The hash of a
key is a plain 64-bit SUM of one word per (locus, mask) pair, so "two pairs against two pairs" is a four-list sum problem (Wagner's
generalised birthday): with lists V1 .. V4 of pair words, find  V1[i] + V3[k] == V2[j] + V4[l]  (mod 2^64).  Join V1 with V2 on the low
BITS bits of V1 - V2 == 0, join V4 with V3 the same way, then match the two lists of differences on all 64 bits.  Lists of 2^23 words
joined on 23 bits leave about 2^23 differences on each side and 41 bits to match: some tens of hits.  The sums are matched exactly (bit 0
included, which ``finish_hash`` would forgive), so that the same padding pairs added to both keys keep the hashes equal whatever they sum to.

Families (every locus of a differing pair lies in [65536, 229376); the loci below and above are left for padding pairs):

  F2    {a, b} against {c, d}: four different loci, one from each of four blocks of 2^15 loci, masks 1 .. 255 (8 haplotypes)
  M2    {(l1, m1), (l2, m2)} against {(l1, m1'), (l2, m2')}: the SAME two loci, masks below 2^24 (24 haplotypes; m below 2^23 on one
        side and from 2^23 up on the other, so that they differ by construction)
  N23   {a, b} against {c, d, e}: e a fixed pair of a fifth block, its word and the n * (2^32 + 1) difference of finish_hash folded into
        the fourth list as a constant

    python tests/golden/make_hash_collisions.py

Measured (numpy, one CPU thread, lists of 2^23): F2 26 hits in 64 s; M2 29 and 39 hits in 62 s and 66 s (two pairs of loci); N23 31 and
23 hits in 74 s and 69 s (two third pairs): 5.6 minutes in all.  The first KEEP hits of each search are committed."""
from __future__ import print_function

import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import set_hash as sh  # noqa: E402

BITS = 23
BASE, BLOCK = 65536, 1 << 15
N_LOCI = 1 << 18
PAD_LOW, PAD_HIGH = [1, BASE], [BASE + 5 * BLOCK, N_LOCI]
KEEP = 8                                     # instances committed per search


def join(va, vb):
    """(ia, ib) of every pair with va[ia] - vb[ib] == 0 modulo 2^BITS."""
    m = np.uint64((1 << BITS) - 1)
    ka, kb = va & m, vb & m
    ob = np.argsort(kb, kind="stable")
    kbs = kb[ob]
    lo, hi = np.searchsorted(kbs, ka, "left"), np.searchsorted(kbs, ka, "right")
    cnt = hi - lo
    ia = np.repeat(np.arange(len(va)), cnt)
    within = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return ia, ob[np.repeat(lo, cnt) + within]


def four_list(v1, v2, v3, v4):
    """[(i, j, k, l)] with v1[i] + v3[k] == v2[j] + v4[l] modulo 2^64."""
    with np.errstate(over="ignore"):
        i, j = join(v1, v2)
        d12 = v1[i] - v2[j]
        l, k = join(v4, v3)
        d43 = v4[l] - v3[k]
        _, x, y = np.intersect1d(d12, d43, return_indices=True)
    return [(int(i[a]), int(j[a]), int(k[b]), int(l[b])) for a, b in zip(x, y)]


def block_list(b):
    """Every (locus, mask) of block b with masks 1 .. 255."""
    loci = np.repeat(BASE + b * BLOCK + np.arange(BLOCK, dtype=np.int64), 255)
    masks = np.tile(np.arange(1, 256, dtype=np.int64), BLOCK)
    return loci, masks


def search_f2(extra=None):
    """F2, or N23 when `extra` = (locus, mask) of the third pair of key b."""
    (l1, m1), (l3, m3), (l2, m2), (l4, m4) = (block_list(b) for b in range(4))        # a, b from blocks 0, 1; c, d from blocks 2, 3
    v = [sh.pair_hash64(l, m) for l, m in ((l1, m1), (l2, m2), (l3, m3), (l4, m4))]
    if extra is not None:
        with np.errstate(over="ignore"):
            v[3] = v[3] + sh.pair_hash64([extra[0]], [extra[1]])[0] + np.uint64(sh.N_TERM)        # sum(a) + 2 K == sum(b) + 3 K
    out = []
    for i, j, k, l in four_list(*v):
        a = [[int(l1[i]), int(m1[i])], [int(l3[k]), int(m3[k])]]
        b = [[int(l2[j]), int(m2[j])], [int(l4[l]), int(m4[l])]] + ([list(extra)] if extra is not None else [])
        out.append({"a": a, "b": b})
    return out


def search_m2(loc1, loc2):
    half = 1 << 23
    lo_m, hi_m = np.arange(1, half, dtype=np.int64), np.arange(half, 2 * half, dtype=np.int64)
    v1, v2 = sh.pair_hash64(np.full(len(lo_m), loc1), lo_m), sh.pair_hash64(np.full(len(hi_m), loc1), hi_m)
    v3, v4 = sh.pair_hash64(np.full(len(lo_m), loc2), lo_m), sh.pair_hash64(np.full(len(hi_m), loc2), hi_m)
    return [{"a": [[loc1, int(lo_m[i])], [loc2, int(lo_m[k])]], "b": [[loc1, int(hi_m[j])], [loc2, int(hi_m[l])]]}
            for i, j, k, l in four_list(v1, v2, v3, v4)]


def timed(what, f, *args):
    t0 = time.time()
    hits = f(*args)
    for c in hits:                                                  # every hit re-checked with the whole hash, key by key
        ha, hb = (sh.set_hash([p[0] for p in c[s]], [p[1] for p in c[s]]) for s in ("a", "b"))
        assert ha == hb and c["a"] != c["b"], c
        c["hash"] = "0x%016x" % ha
    print("%s: %d hits in %.0f s" % (what, len(hits), time.time() - t0))
    assert len(hits) >= 3, "enlarge the lists"
    return hits[:KEEP]


def main():
    fam = {}
    fam["F2"] = {"n_haps": 8, "collisions": timed("F2", search_f2)}
    fam["M2"] = {"n_haps": 24, "collisions": timed("M2 (70001, 150001)", search_m2, 70001, 150001)
                 + timed("M2 (99999, 100000)", search_m2, 99999, 100000)}
    e_block = BASE + 4 * BLOCK
    fam["N23"] = {"n_haps": 8, "collisions": timed("N23 e low", search_f2, (e_block + 17, 0x81))
                  + timed("N23 e high", search_f2, (e_block + BLOCK - 5, 0x3c))}
    with open(os.path.join(HERE, "hash_collisions.json"), "w") as f:               # (one collision per line)
        f.write('{"n_loci":%d,"pad_low":%s,"pad_high":%s,"families":{\n' % (N_LOCI, json.dumps(PAD_LOW), json.dumps(PAD_HIGH)))
        f.write(",\n".join('"%s":{"n_haps":%d,"collisions":[\n%s\n]}' % (name, d["n_haps"], ",\n".join(json.dumps(c, separators=(",", ":"))
                                                                                                  for c in d["collisions"]))
                           for name, d in fam.items()))
        f.write("\n}}\n")


if __name__ == "__main__":
    main()
