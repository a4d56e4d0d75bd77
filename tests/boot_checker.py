"""ecboot's yardstick, in numpy and Python integers: Philox4x32-10 as Random123 defines it, the map of a draw onto ``[0, W)``, a replicate's
counts by ``searchsorted`` and ``bincount``, the dense scatter of a sparse per-replicate answer and Welford's loop over the replicates.
Nothing here is taken from the library: it restates ``include/ecb_quant_boot.h``."""
import numpy as np

import counts_checker

M0, M1 = 0xD2511F53, 0xCD9E8D57
K0, K1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox(counter, key):
    """Philox4x32-10 of four counter words and two key words -> four words.  Every argument an int, or uint64 arrays of one shape."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(MASK) for c in counter)
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    sh, mask = np.uint64(32), np.uint64(MASK)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # (32 x 32 bits: no overflow of the 64)
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ np.uint64(k0), p1 & mask, (p0 >> sh) ^ c3 ^ np.uint64(k1), p0 & mask
        k0, k1 = (k0 + K0) & MASK, (k1 + K1) & MASK
    return c0, c1, c2, c3


def draws_u(seed, b, W):
    """u of draws 0 .. W - 1 of replicate b: a list of Python integers below 2^64."""
    j = np.arange((W + 1) // 2, dtype=np.uint64)
    z = np.zeros_like(j)
    o0, o1, o2, o3 = philox((j, z, z + np.uint64(b), z), (seed & MASK, seed >> 32))
    u = np.empty(2 * len(j), dtype=object)
    u[0::2] = [(int(h) << 32) | int(l) for h, l in zip(o1, o0)]
    u[1::2] = [(int(h) << 32) | int(l) for h, l in zip(o3, o2)]
    return list(u[:W])


def draw_x(seed, b, i, W):
    """x of draw i of replicate b, in Python integers."""
    o = [int(v) for v in philox((i >> 1, 0, b, 0), (seed & MASK, seed >> 32))]
    u = (o[3] << 32 | o[2]) if i & 1 else (o[1] << 32 | o[0])
    return (u * W) >> 64


def xs(seed, b, W):
    """x of every draw of replicate b: int64 [W]."""
    return np.array([(u * W) >> 64 for u in draws_u(seed, b, W)], dtype=np.int64)


def weights(n_ecs, indptr_n, indices_n, data_n, sample=None):
    return np.asarray(counts_checker.weights(n_ecs, indptr_n, indices_n, data_n, sample), dtype=np.int64)


def replicate(w, seed, b):
    """n_b[e] of replicate b over the weights w: int64 [E]; a draw lands on the row e with cum[e - 1] <= x < cum[e]."""
    cum = np.cumsum(w)
    W = int(cum[-1]) if len(cum) else 0
    if not W:
        return np.zeros(len(w), dtype=np.int64)
    return np.bincount(np.searchsorted(cum, xs(seed, b, W), side="right"), minlength=len(w)).astype(np.int64)


def resample(w, seed, b0, n_reps):
    """The CSC N ecb_resample returns: (rep_ptr, rep_ec, rep_count) int32, and the dense counts [n_reps, E]."""
    dense = np.array([replicate(w, seed, b0 + r) for r in range(n_reps)], dtype=np.int64).reshape(n_reps, len(w))
    ptr, ec, cnt = [0], [], []
    for n in dense:
        rows = np.flatnonzero(n)
        ec.append(rows)
        cnt.append(n[rows])
        ptr.append(ptr[-1] + len(rows))
    cat = lambda v: np.concatenate(v).astype(np.int32) if v else np.zeros(0, dtype=np.int32)
    return np.array(ptr, dtype=np.int32), cat(ec), cat(cnt), dense


def z_statistic(dense, w):
    """(chi^2 - k) / sqrt(2 k) of the issue: chi^2 = the sum over the k rows with weight of B (mean_b n_b[e] - w[e])^2 / (w[e] (1 - w[e] / W))."""
    w = np.asarray(w, dtype=np.float64)
    B, W = dense.shape[0], w.sum()
    rows = w > 0
    k = int(rows.sum())
    chi2 = float((B * (dense[:, rows].mean(axis=0) - w[rows]) ** 2 / (w[rows] * (1.0 - w[rows] / W))).sum())
    return (chi2 - k) / np.sqrt(2.0 * k)


def scatter(cell_ptr, slot_locus, theta, n_loci, n_haps):
    """The sparse answer of ecb.quantify_cells -> dense [cells, H, T], 0 outside every cell's support."""
    S = len(cell_ptr) - 1
    out = np.zeros((S, n_haps, n_loci), dtype=np.float64)
    for c in range(S):
        a, b = int(cell_ptr[c]), int(cell_ptr[c + 1])
        out[c][:, slot_locus[a:b]] = theta[a:b].T
    return out


def welford(x):
    """x [B, ...] -> (mean, sd) over axis 0, in replicate order: d = x_b - m; m += d / (b + 1); M += d (x_b - m); sd = sqrt(M / (B - 1))."""
    m, M = np.zeros(x.shape[1:]), np.zeros(x.shape[1:])
    for b in range(x.shape[0]):
        d = x[b] - m
        m = m + d / (b + 1)
        M = M + d * (x[b] - m)
    B = x.shape[0]
    return m, (np.sqrt(M / (B - 1)) if B > 1 else np.zeros_like(M)), M


def totals(x):
    """y_b[t] = the sum over h of x_b[h, t], h ascending: [B, T]."""
    y = np.zeros((x.shape[0], x.shape[2]))
    for h in range(x.shape[1]):
        y = y + x[:, h, :]
    return y
