"""CHECKER (test infrastructure): which reads of a perturbed tuple stream no longer have the target set they were pushed with -- what
libecb's exactness pass (``ecb_verify_device`` / ``ecb_verify_device_tiled``) must count.  Sorted numpy keys; nothing here comes from libecb."""
from itertools import chain

import numpy as np

from oracle import ec_oracle as orc


def target_sets(t, n_haps):
    """The stream's (read, locus, mask) triples, sorted, one per (read, locus): mask = OR of ``1 << hap`` over the read's records on the
    locus that pass ``orc.tuples_valid``."""
    hf = np.asarray(t["hapflag"]).astype(np.int64)
    ok = orc.tuples_valid(hf)
    rid = np.asarray(t["read_id"]).astype(np.int64)[ok]
    loc = np.asarray(t["locus"]).astype(np.int64)[ok]
    hap = (hf[ok] >> 16) & 0xFF
    assert len(hap) == 0 or int(hap.max()) < n_haps
    o = np.lexsort((loc, rid))
    rid, loc, bit = rid[o], loc[o], np.int64(1) << hap[o]
    head = np.ones(len(rid), bool)
    head[1:] = (rid[1:] != rid[:-1]) | (loc[1:] != loc[:-1])
    starts = np.flatnonzero(head)
    mask = np.bitwise_or.reduceat(bit, starts) if len(starts) else bit[:0]
    return rid[starts], loc[starts], mask


def misplaced(t, t2, n_haps):
    """-> bool array over the reads: read r is misplaced iff its target set {locus -> OR of 1 << hap over its valid records} under ``t2``
    differs from its set under ``t`` (the stream that was pushed; ``t2`` has the same length and the same ``read_id`` array)."""
    assert np.array_equal(t["read_id"], t2["read_id"])
    n_reads = int(np.asarray(t["read_id"]).max()) + 1 if len(t["read_id"]) else 0
    a, b = target_sets(t, n_haps), target_sets(t2, n_haps)
    # a (read, locus, mask) triple is in each stream at most once: sorted together, one that the two streams share sits next to its twin
    r, l, m = (np.concatenate([x, y]) for x, y in zip(a, b))
    o = np.lexsort((m, l, r))
    r, l, m = r[o], l[o], m[o]
    twin = (r[1:] == r[:-1]) & (l[1:] == l[:-1]) & (m[1:] == m[:-1])
    shared = np.zeros(len(r), bool)
    shared[1:] |= twin
    shared[:-1] |= twin
    out = np.zeros(n_reads, bool)
    out[r[~shared]] = True
    return out


# ---- perturbations that keep the tuple contract ---------------------------------------------------------------------------------------------
#: ways to change one read: the first seven change its target set, the last two change its records only
COUNTED = ("hap", "locus", "drop", "new_locus", "new_bit", "hap_highest", "hap_lowest")
NOT_COUNTED = ("permute", "dup")
KINDS = COUNTED + NOT_COUNTED


def perturb(t, r, kind, n_loci, n_haps):
    """``t`` with read ``r`` changed in one way, or None where the read has not got the records that way needs.  The result shares
    ``read_id`` (and whichever of ``locus`` / ``hapflag`` stays as it is) with ``t``; the read's head record stays valid, loci stay below
    ``n_loci`` and haplotypes below ``n_haps``.
      hap          one valid record's haplotype becomes one its locus has not got in this read
      locus        one valid record's locus becomes one that no record of the read is on
      drop         one valid record behind the head that alone carries its locus gets flag 0x4
      new_locus    one invalid record behind the head becomes valid, on a locus that no record of the read is on
      new_bit      one invalid record behind the head becomes valid, on a locus the read holds, with a haplotype it has not got there
      hap_highest  `hap` on a valid record of the read's highest locus (the last pair of the stored key) ...
      hap_lowest   ... and of its lowest (the first)
      permute      the records behind the head in reverse order
      dup          one invalid record behind the head becomes a copy of a valid record of the read"""
    rid, loc, hf = t["read_id"], t["locus"], t["hapflag"]
    a, z = (int(x) for x in np.searchsorted(rid, [r, r + 1]))
    ok = orc.tuples_valid(hf[a:z])
    assert z > a and ok[0]
    L, hap = loc[a:z].astype(np.int64), (hf[a:z].astype(np.int64) >> 16) & 0xFF
    v = [i for i in range(1, z - a) if ok[i]]                    # valid / invalid records behind the head
    u = [i for i in range(1, z - a) if not ok[i]]
    mask = {}
    for i in np.flatnonzero(ok):
        mask[int(L[i])] = mask.get(int(L[i]), 0) | (1 << int(hap[i]))
    on = set(L.tolist())
    fresh = next((x for x in chain(range(int(L.max()) + 1, n_loci), range(int(L.min()) - 1, -1, -1)) if x not in on), None)

    def missing(locus):
        return next((h for h in range(n_haps) if not mask[locus] >> h & 1), None)
    loc2, hf2 = loc.copy(), hf.copy()
    if kind in ("hap", "hap_highest", "hap_lowest"):
        if kind == "hap":
            i = v[len(v) // 2] if v else 0
        else:
            want = max(mask) if kind == "hap_highest" else min(mask)
            i = next(int(k) for k in np.flatnonzero(ok) if L[k] == want)
        h = missing(int(L[i]))
        if h is None:
            return None
        hf2[a + i] = (int(hf[a + i]) & 0xFFFF) | (h << 16)
    elif kind == "locus":
        if fresh is None:
            return None
        loc2[a + (v[len(v) // 2] if v else 0)] = fresh
    elif kind == "drop":
        alone = [i for i in v if int((L[ok] == L[i]).sum()) == 1]
        if not alone:
            return None
        hf2[a + alone[len(alone) // 2]] |= 0x4
    elif kind == "new_locus":
        if not u or fresh is None:
            return None
        loc2[a + u[0]], hf2[a + u[0]] = fresh, int(hap[u[0]]) << 16
    elif kind == "new_bit":
        room = [(x, missing(x)) for x in sorted(mask) if missing(x) is not None]
        if not u or not room:
            return None
        x, h = room[len(room) // 2]
        loc2[a + u[-1]], hf2[a + u[-1]] = x, h << 16
    elif kind == "permute":
        loc2[a + 1:z], hf2[a + 1:z] = loc[a + 1:z][::-1], hf[a + 1:z][::-1]
    elif kind == "dup":
        if not u:
            return None
        j = v[-1] if v else 0
        loc2[a + u[0]], hf2[a + u[0]] = loc[a + j], hf[a + j]
    else:
        raise ValueError(kind)
    same_l, same_h = np.array_equal(loc2, loc), np.array_equal(hf2, hf)
    if same_l and same_h:
        return None                                               # (nothing to permute, ...)
    out = dict(t)
    out["locus"], out["hapflag"] = (loc if same_l else loc2), (hf if same_h else hf2)
    return out
