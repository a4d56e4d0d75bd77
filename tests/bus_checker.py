"""bus2ec's rule restated in plain Python / numpy -- dicts of molecules, ``set.intersection``, first-appearance numbering, selection -- with a
writer of BUS directories and ``bus_from_bin``, which turns a loaded ``.bin`` into a BUS directory that must convert back to it.  This file
is the definition the GPU tests compare with; ``tests/test_bus2ec.py`` holds it to a hand-written case."""
import collections
import os
import struct

import numpy as np

BASES = "ACGT"


def encode(seq):
    v = 0
    for c in seq:
        v = v * 4 + BASES.index(c)
    return v


def decode(value, length):
    return "".join(BASES[(int(value) >> (2 * (length - 1 - k))) & 3] for k in range(length))


def records(barcodes, umis, ecs, counts, flags=0):
    """The records as bytes: uint8 [n, 32]."""
    rec = np.zeros(len(barcodes), dtype=[("bc", "<u8"), ("umi", "<u8"), ("ec", "<i4"), ("count", "<u4"), ("flags", "<u4"), ("pad", "<u4")])
    rec["bc"], rec["umi"], rec["ec"], rec["count"], rec["flags"] = barcodes, umis, ecs, counts, flags
    return rec.view(np.uint8).reshape(-1, 32)


def fields(rec):
    """(barcodes, umis, ecs, counts) of records()' bytes, as lists of Python ints."""
    r = np.ascontiguousarray(rec).reshape(-1).view([("bc", "<u8"), ("umi", "<u8"), ("ec", "<i4"), ("count", "<u4"), ("flags", "<u4"), ("pad", "<u4")])
    return [[int(x) for x in r[k]] for k in ("bc", "umi", "ec", "count")]


def csr_lines(lines):
    """matrix.ec's lines (lists of target ids) -> (ec_ptr uint32, ec_targets uint32)."""
    ptr = np.concatenate(([0], np.cumsum([len(x) for x in lines]))).astype(np.uint32)
    ids = np.array([t for x in lines for t in x], dtype=np.uint32)
    return ptr, ids


def write_bus_dir(path, rec, bclen, umilen, lines, names, text=b"made by tests/bus_checker.py", version=1):
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "output.bus"), "wb") as fh:
        fh.write(b"BUS\0" + struct.pack("<4I", version, bclen, umilen, len(text)) + text + np.ascontiguousarray(rec).tobytes())
    with open(os.path.join(path, "matrix.ec"), "w") as fh:
        fh.write("".join("%d\t%s\n" % (i, ",".join(str(t) for t in x)) for i, x in enumerate(lines)))
    with open(os.path.join(path, "transcripts.txt"), "w") as fh:
        fh.write("".join(n + "\n" for n in names))
    return path


def _row(targets, tcol, thap):
    """A target set -> ((columns ascending), (masks)): per column the sum of 2^h."""
    m = collections.defaultdict(int)
    for t in targets:
        m[int(tcol[t])] += 1 << int(thap[t])
    cols = sorted(m)
    return tuple(cols), tuple(m[c] for c in cols)


Molecules = collections.namedtuple("Molecules", "barcodes rows row_line N sizes")


def molecules(rec, lines, tcol, thap, keep=None, no_umi=False):
    """What ``ecb_bus_molecules`` returns: the cells, the rows handed on (each ``(columns, masks)``), the line every row came from (-1: a new
    row), N as a dict ``(row, cell) -> count``, and out_sizes."""
    bc, umi, ec, cnt = fields(rec)
    kept = None if keep is None else set(int(b) for b in keep)
    take = [i for i in range(len(bc)) if kept is None or bc[i] in kept]
    cells = sorted(set(bc[i] for i in take))
    cid = {b: c for c, b in enumerate(cells)}
    line_events, new_rows, new_events = collections.Counter(), [], []
    n_mol = n_multi = n_disc = 0
    if no_umi:
        for i in take:
            if cnt[i]:
                line_events[(ec[i], cid[bc[i]])] += cnt[i]
                n_mol += 1
    else:
        mols = collections.defaultdict(set)
        for i in take:
            mols[(bc[i], umi[i])].add(ec[i])
        n_mol = len(mols)
        for (b, u) in sorted(mols):
            es = sorted(mols[(b, u)])
            if len(es) == 1:
                line_events[(es[0], cid[b])] += 1
                continue
            n_multi += 1
            inter = set.intersection(*[set(lines[e]) for e in es])
            if not inter:
                n_disc += 1
                continue
            new_events.append((len(new_rows), cid[b]))
            new_rows.append(sorted(inter))
    used = sorted(set(e for e, _ in line_events))
    lrow = {e: r for r, e in enumerate(used)}
    rows = [_row(lines[e], tcol, thap) for e in used] + [_row(t, tcol, thap) for t in new_rows]
    N = {(lrow[e], c): v for (e, c), v in line_events.items()}
    for s, c in new_events:
        N[(len(used) + s, c)] = 1
    nnz_a = sum(len(r[0]) for r in rows)
    return Molecules(cells, rows, used + [-1] * len(new_rows), N, (len(cells), len(rows), nnz_a, len(N), n_mol, n_multi, n_disc, len(new_rows)))


def csr(rows):
    ip = np.concatenate(([0], np.cumsum([len(r[0]) for r in rows]))).astype(np.int32)
    return ip, np.array([c for r in rows for c in r[0]], dtype=np.int32), np.array([m for r in rows for m in r[1]], dtype=np.int32)


def csc(N, n_cols):
    """A dict (row, column) -> count as CSC: rows ascending within a column."""
    cols = [[] for _ in range(n_cols)]
    for (r, c) in sorted(N):
        cols[c].append((r, N[(r, c)]))
    ip = np.concatenate(([0], np.cumsum([len(x) for x in cols]))).astype(np.int32)
    return ip, np.array([r for x in cols for r, _ in x], dtype=np.int32), np.array([v for x in cols for _, v in x], dtype=np.int32)


Result = collections.namedtuple("Result", "A N samples stats")


def bus2ec(rec, bclen, lines, tcol, thap, names=None, mincount=1000, no_umi=False):
    """The whole rule: ``names`` = [(barcode value, sample name)] in the file's order or None.  -> Result(CSR A, CSC N, sample names,
    stats dict), or ValueError("no sample left")."""
    mol = molecules(rec, lines, tcol, thap, keep=None if names is None else [b for b, _ in names], no_umi=no_umi)
    if names is None:
        snames, smap = [decode(b, bclen) for b in mol.barcodes], list(range(len(mol.barcodes)))
    else:
        where = {b: k for k, (b, _) in enumerate(names)}
        snames, smap = [n for _, n in names], [where[b] for b in mol.barcodes]
    if not mol.barcodes:
        raise ValueError("no sample left")
    # combine: equal keys become one EC, numbered by first appearance; N summed
    ec_of_key, ec_of_row = {}, []
    for r in mol.rows:
        ec_of_row.append(ec_of_key.setdefault(r, len(ec_of_key)))
    line_keys = len(set(r for r, l in zip(mol.rows, mol.row_line) if l >= 0))
    N = collections.Counter()
    for (r, c), v in mol.N.items():
        N[(ec_of_row[r], smap[c])] += v
    keys = list(ec_of_key)
    # select: the samples that count max(m, 1); the rows that keep a read, renumbered
    total = collections.Counter()
    for (e, s), v in N.items():
        total[s] += v
    stay = [total[s] >= max(mincount, 1) for s in range(len(snames))]
    new_s = np.cumsum(stay) - 1
    left = {(e, s): v for (e, s), v in N.items() if stay[s] and v > 0}
    rows_left = sorted(set(e for e, _ in left))
    new_e = {e: k for k, e in enumerate(rows_left)}
    out_n = {(new_e[e], int(new_s[s])): v for (e, s), v in left.items()}
    samples = [n for n, k in zip(snames, stay) if k]
    if not samples:
        raise ValueError("no sample left")
    stats = dict(records=len(np.ascontiguousarray(rec).reshape(-1)) // 32, molecules=mol.sizes[4], molecules_in_several_ecs=mol.sizes[5],
                 molecules_discarded=mol.sizes[6], new_ecs=len(keys) - line_keys, cells=len(mol.barcodes), cells_kept=len(samples))
    return Result(csr([keys[e] for e in rows_left]), csc(out_n, len(samples)), samples, stats)


def bus_from_bin(m, path, seed=0, bclen=16, umilen=12, split=False, shuffle=False, triple=False, no_umi=False):
    """A loaded ``.bin`` as a BUS directory that converts back to it: target ``t * H + h`` is named ``lname_hname``, line e of matrix.ec holds
    the targets of row e of A, every read is a record with a UMI of its own in its cell (``no_umi``: one record per non-zero of N carrying its
    count), and the cells' barcodes are random, not in sample order.  ``split``: every third read -- never the first of its EC, so that every
    line still receives a read of its own and the ECs keep their numbering -- becomes two records of one UMI naming two wider ECs appended to
    matrix.ec, the read's targets plus one foreign target each, whose intersection is the read's EC.  ``shuffle``: the records in random
    order.  ``triple``: every record three times.  -> dict(dir, names, lengths): the directory, and the files for ``--names`` and ``-l``."""
    rng = np.random.default_rng(seed)
    H, T, S = m.num_haplotypes, m.num_loci, m.num_samples
    names = ["%s_%s" % (l, h) for l in m.lname for h in m.hname]
    lines = []
    for e in range(m.num_reads):
        a, b = m.indptrA[e], m.indptrA[e + 1]
        lines.append([int(c) * H + h for c, mask in zip(m.indicesA[a:b], m.dataA[a:b]) for h in range(H) if (int(mask) >> h) & 1])
    values = rng.choice(1 << 20, size=S, replace=False).astype(np.uint64) * np.uint64(4093) + np.uint64(7)      # (below 4^16, distinct, unordered)
    wide = {}
    bc, umi, ec, cnt = [], [], [], []
    seen_ec, read_no = set(), 0
    for s in range(S):
        u = 0
        for k in range(m.indptrN[s], m.indptrN[s + 1]):
            e, c = int(m.indicesN[k]), int(m.dataN[k])
            if no_umi:
                bc.append(values[s]); umi.append(0); ec.append(e); cnt.append(c)
                continue
            for _ in range(c):
                read_no += 1
                if split and read_no % 3 == 0 and e in seen_ec:
                    if e not in wide:
                        foreign = [t for t in range(T * H) if t not in set(lines[e])][:2]
                        wide[e] = (len(lines), len(lines) + 1)
                        lines += [sorted(lines[e] + [f]) for f in foreign]
                    for w in wide[e]:
                        bc.append(values[s]); umi.append(u); ec.append(w); cnt.append(1)
                else:
                    bc.append(values[s]); umi.append(u); ec.append(e); cnt.append(1)
                seen_ec.add(e)
                u += 1
    rec = records(np.array(bc, dtype=np.uint64), np.array(umi, dtype=np.uint64), ec, cnt)
    if triple:
        rec = np.repeat(rec, 3, axis=0)
    if shuffle:
        rec = rec[rng.permutation(len(rec))]
    write_bus_dir(path, rec, bclen, umilen, lines, names)
    out = dict(dir=path, names=os.path.join(path, "names.txt"), lengths=os.path.join(path, "lengths.txt"), records=rec, lines=lines, values=values)
    with open(out["names"], "w") as fh:
        fh.write("".join("%s\t%s\n" % (decode(v, bclen), n) for v, n in zip(values, m.sname)))
    with open(out["lengths"], "w") as fh:
        fh.write("".join("%s_%s\t%d\n" % (l, h, int(m.lengths[t, k])) for t, l in enumerate(m.lname) for k, h in enumerate(m.hname)))
    return out
