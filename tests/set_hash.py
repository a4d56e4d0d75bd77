"""The EC-table's set hash (``alntools_amd/csrc/ecb.hip``: fmix32, pair_hash64, finish_hash) restated in numpy, and helpers that turn
the committed collisions of ``tests/golden/hash_collisions.json`` (made by ``tests/golden/make_hash_collisions.py``) into keys and reads.
``test_hash_collisions.py`` pins the constants below against the kernel source; ``test_gpu_hash_collisions.py`` ties the restatement to
the device through ``export_ec_keys_device``.

The hash of a key {locus -> mask} of n pairs is ``(sum of pair_hash64(locus, mask) + n * (2^32 + 1)) | 1`` in 64-bit arithmetic.  A
committed collision is two different keys whose SUMS are equal modulo 2^64 when both have the same number of pairs, or differ by exactly
the ``n * (2^32 + 1)`` term when they do not: adding the same pairs to both keeps the hashes equal, whatever the pairs."""
import json
import os

import numpy as np

M32 = 0xFFFFFFFF
FMIX_MUL1, FMIX_MUL2 = 0x85EBCA6B, 0xC2B2AE35          # fmix32: h ^= h >> 16; h *= MUL1; h ^= h >> 13; h *= MUL2; h ^= h >> 16
MUL_LOCUS, MUL_MASK, ADD0 = 0x9E3779B1, 0x85EBCA77, 0x7F4A7C15   # h0 = fmix32(locus * MUL_LOCUS + mask * MUL_MASK + ADD0)
MUL_H1 = 0xC2B2AE3D                                     # h1 = fmix32((h0 ^ locus) * MUL_H1 + mask)
N_TERM = (1 << 32) + 1                                  # finish_hash: (s0 + ((u64)n << 32) + n) | 1

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hash_collisions.json")


def fmix32(h):
    h = np.asarray(h, np.uint64) & np.uint64(M32)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(FMIX_MUL1)) & np.uint64(M32)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(FMIX_MUL2)) & np.uint64(M32)
    h ^= h >> np.uint64(16)
    return h


def pair_hash64(locus, mask):
    """uint64 array: the 64-bit word of every (locus, mask) pair (32-bit arithmetic carried in the low halves of 64-bit words)."""
    locus = np.asarray(locus, np.uint64) & np.uint64(M32)
    mask = np.asarray(mask, np.uint64) & np.uint64(M32)
    m = np.uint64(M32)
    h0 = fmix32(((locus * np.uint64(MUL_LOCUS)) & m) + ((mask * np.uint64(MUL_MASK)) & m) + np.uint64(ADD0))
    h1 = fmix32(((((h0 ^ locus) & m) * np.uint64(MUL_H1)) & m) + mask)
    return (h1 << np.uint64(32)) | h0


def finish_hash(s0, n):
    return (int(s0) + int(n) * N_TERM) % (1 << 64) | 1


def set_hash(loci, masks):
    """The table hash of one key, as a Python int."""
    with np.errstate(over="ignore"):
        s0 = int(np.sum(pair_hash64(loci, masks), dtype=np.uint64)) if len(loci) else 0
    return finish_hash(s0, len(loci))


def row_hashes(indptr, indices, data):
    """The table hash of every row of a CSR matrix of keys (indices = loci, data = masks): uint64 array."""
    return np.array([set_hash(indices[a:z], data[a:z]) for a, z in zip(indptr[:-1], indptr[1:])], dtype=np.uint64)


def load():
    """The fixture: {"n_loci", "pad_low": [lo, hi), "pad_high": [lo, hi), "families": {name: {"n_haps", "collisions": [{"a", "b"}]}}}, keys as
    lists of [locus, mask]."""
    with open(FIXTURE) as f:
        return json.load(f)


def pad(collision, n, where, fx=None):
    """Both keys of `collision` extended with the SAME padding pairs until key a has n pairs (key b then has n too, n + 1 in family N23) ->
    (key_a, key_b), each a (loci, masks) pair of int64 arrays sorted by locus.  where: the differing pairs hold the "low"est, "mid"dle or
    "high"est loci of the padded keys.  The padding loci come from the two ranges the search left free of differing loci (below and above
    them); their masks are single haplotype bits below 256."""
    fx = fx or load()
    a, b = np.array(collision["a"], np.int64).reshape(-1, 2), np.array(collision["b"], np.int64).reshape(-1, 2)
    k = n - len(a)
    assert k >= 0 and len(a) <= len(b) and where in ("low", "mid", "high")
    n_below = {"low": 0, "mid": k // 2, "high": k}[where]
    (l0, l1), (h0, h1) = fx["pad_low"], fx["pad_high"]
    assert n_below <= l1 - l0 and k - n_below <= h1 - h0
    # deterministic and spread: every 7th locus up from the range's start (below), every 5th (above)
    step_lo, step_hi = max(1, min(7, (l1 - l0) // max(1, n_below))), max(1, min(5, (h1 - h0) // max(1, k - n_below)))
    ploci = np.concatenate([l0 + step_lo * np.arange(n_below), h0 + step_hi * np.arange(k - n_below)]).astype(np.int64)
    pmask = (1 << (ploci * 3 % 8)).astype(np.int64)
    out = []
    for key in (a, b):
        loci, masks = np.concatenate([key[:, 0], ploci]), np.concatenate([key[:, 1], pmask])
        o = np.argsort(loci, kind="stable")
        out.append((loci[o], masks[o]))
    return tuple(out)


def read_of(key, order="asc"):
    """One read whose target set is `key` = (loci, masks): a record per set haplotype bit -> (loci, haps) record arrays.  order: the loci
    ascending or descending within the read (the records of one locus stay together)."""
    loci, masks = key
    rl, rh = [], []
    idx = range(len(loci)) if order == "asc" else range(len(loci) - 1, -1, -1)
    for i in idx:
        m = int(masks[i])
        for h in range(32):
            if m >> h & 1:
                rl.append(int(loci[i]))
                rh.append(h)
    return np.array(rl, np.int64), np.array(rh, np.int64)


# ---- displaced pairs: the stream kernel's LDS place of a locus (k_stream.inc: pack_lgf, home_off) ----------------------------------------------
def home_off(locus, g=3):
    """The place of `locus` within its read's home region of 1 << g LDS slots: bits [16, 16 + g) of (locus + 1) * fmul in 24 x 24 -> 32 bit
    arithmetic, fmul = the sum of 2^16 >> (i * g) over i = 0 .. 5.  g = 3 (eight slots) is what a pass laid out for the most reads it can
    take has: ``pack_lgf(LGMAX)`` at a slice's start, and behind every flush whose last tile brought 16 reads (ks_std, ks_par) or 32
    (ks_short) and more (``min(est * ECB_EST_MUL, 1 << LGMAX)``)."""
    fmul = sum((1 << 16) >> (i * g) for i in range(6)) & 0xFFFFFF
    return ((((int(locus) + 1) & 0xFFFFFF) * fmul) & 0xFFFFFFFF) >> 16 & ((1 << g) - 1)


def displace(collision, n, founder, where="mid", fx=None):
    """`pad(collision, n - k, where)` plus k displacing pairs, the same in both keys: for every differing locus D of the founder's key (k = its
    number of differing pairs; founder "a" or "b") or of both keys ("ab") one padding locus P with home_off(P) == home_off(D) at g = 3.  In
    the pass table of the OTHER key's read, which holds P and not D, the first place of D is then taken by another (read, locus): a lookup
    that meets the founder's stored key cannot tell from D's first place and must walk on.  -> (key_a, key_b) as `pad` gives them."""
    fx = fx or load()
    a, b = collision["a"], collision["b"]
    common = {tuple(p) for p in a} & {tuple(p) for p in b}
    want = [p[0] for s, key in (("a", a), ("b", b)) if s in founder for p in key if tuple(p) not in common]
    (l0, l1), (h0, h1) = fx["pad_low"], fx["pad_high"]
    ka, kb = pad(collision, n - len(want), where, fx)
    taken, disp = set(ka[0].tolist()) | set(kb[0].tolist()), []
    for k, d in enumerate(want):                  # (a stretch of loci takes seven of the eight places: both padding ranges are searched)
        cand = list(range(l0 + 20000 + 1000 * k, l1)) + list(range(h0 + 20000, h1)) + list(range(l0 + 10000, l0 + 20000))
        p = next(x for x in cand if x not in taken and home_off(x) == home_off(d))
        taken.add(p)
        disp.append((p, 1 << (p % 8)))
    out = []
    for loci, masks in (ka, kb):
        loci, masks = np.concatenate([loci, [p for p, _ in disp]]).astype(np.int64), np.concatenate([masks, [m for _, m in disp]]).astype(np.int64)
        o = np.argsort(loci, kind="stable")
        out.append((loci[o], masks[o]))
    return tuple(out)
