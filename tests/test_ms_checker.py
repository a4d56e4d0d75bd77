"""``ms_checker.reduce_triples`` -- the expected result of every multisample GPU test -- against a plain walk of the reference's loop
(bam_utils_multisample.py:503-636, 737-791) in dicts, on small random triples that take both of its sort branches: more than 65 535
cells (the uint32 argsort) and file * n_ecs + ec at or above 2^31 (lexsort instead of the packed key)."""
import numpy as np
import pytest

from ms_checker import reduce_triples


def _walk(tr, n_ecs, minimum_count):
    """cr_totals in insertion order: files in order; within a file the ECs by first appearance there; within an EC its cells by
    first appearance.  Then the minimum count, the EC re-rank and N as CSC over (kept EC, kept cell)."""
    by_file = {}
    for e, c, f, n, r in zip(*(tr[k].tolist() for k in ("ec", "cell", "file", "count", "first"))):
        by_file.setdefault(f, {}).setdefault(e, []).append((r, c, n))
    cr_totals = {}
    for f in sorted(by_file):
        ecs = by_file[f]
        for e in sorted(ecs, key=lambda e: min(ecs[e])[0]):
            for _, c, n in sorted(ecs[e]):
                cr_totals[c] = cr_totals.get(c, 0) + n
    if minimum_count <= 0:
        minimum_count = 1
    kept = [c for c, n in cr_totals.items() if n >= minimum_count]
    col = {c: j for j, c in enumerate(kept)}
    n = {}
    for e, c, cnt in zip(tr["ec"].tolist(), tr["cell"].tolist(), tr["count"].tolist()):
        if c in col:
            n[(e, c)] = n.get((e, c), 0) + cnt
    ec_keep = np.zeros(n_ecs, bool)
    for e, _ in n:
        ec_keep[e] = True
    rank = np.cumsum(ec_keep) - 1
    cols = [sorted((int(rank[e]), v) for (e, c), v in n.items() if c == k) for k in kept]
    indptr = np.concatenate([[0], np.cumsum([len(x) for x in cols])])
    rows = np.array([r for x in cols for r, _ in x], np.int64)
    data = np.array([v for x in cols for _, v in x], np.int64)
    return kept, ec_keep, (indptr, rows, data)


def _triples(rng, n, n_ecs, n_cells, n_files):
    """n distinct (EC, cell, file) triples, sorted so; every triple its own first read (a read is in one triple), counts 1 .. 5."""
    k = np.unique(rng.integers(0, n_ecs, n) * (n_cells * n_files) + rng.integers(0, n_cells, n) * n_files + rng.integers(0, n_files, n))
    ec, rest = k // (n_cells * n_files), k % (n_cells * n_files)
    return dict(ec=ec, cell=rest // n_files, file=rest % n_files, count=rng.integers(1, 6, len(k)),
                first=rng.permutation(10 * len(k))[:len(k)])


@pytest.mark.parametrize("seed,n_ecs,n_cells,n_files", [
    (0, 40, 300, 3),                       # the packed key, the uint16 argsort
    (1, 40, 70_000, 3),                    # more than 65 535 cells
    (2, 3_000_000, 300, 1024),             # file * n_ecs + ec beyond 2^31
    (3, 3_000_000, 100_000, 1024),         # both
    (4, 5, 66_000, 700),                   # few ECs over many files and cells: long walks per (file, EC)
])
def test_checker_equals_a_walk_of_the_reference_loop(seed, n_ecs, n_cells, n_files):
    rng = np.random.default_rng(seed)
    tr = _triples(rng, 3000, n_ecs, n_cells, n_files)
    fe = tr["file"] * n_ecs + tr["ec"]
    assert (int(fe.max()) >= 1 << 31) == (n_ecs * n_files >= 1 << 31)
    totals = np.bincount(tr["cell"], weights=tr["count"]).astype(np.int64)
    for mc in (-1, 0, 1, 2, int(np.quantile(totals[totals > 0], 0.5)) + 1, int(totals.max())):
        kept, ec_keep, (ip, ix, da) = reduce_triples(tr, n_ecs, n_cells, mc)
        w_kept, w_keep, (wip, wix, wda) = _walk(tr, n_ecs, mc)
        assert kept == w_kept, mc
        assert np.array_equal(ec_keep, w_keep)
        assert np.array_equal(ip, wip) and np.array_equal(ix, wix) and np.array_equal(da, wda), mc
