# -*- coding: utf-8 -*-
"""Input and timing of profiles/bus2ec_c4.txt: a synthetic BUS file at config 4's shape -- 5 000 cells with log-normal sizes, the EC
structure of ``alntools_amd/synth.py``'s config-4 reads (80 000 loci, 8 haplotypes, paired: the distinct (locus, haplotype) sets of a
sample of reads are the lines of matrix.ec), about one molecule in ten seen in two ECs (half of those in a line and a wider copy of it, so
that the intersection is the line; half in two unrelated lines, mostly an empty intersection).

    python tools/bus_c4.py [N_RECORDS]       (default 100 000 000)

Reports, from one process: the wall time and the HIP-event time of ``ecb_bus_molecules_device`` on device arrays, warm, five calls each,
with UMIs and without; the same call on a 1/100 slice next to ``tests/bus_checker.py`` on that slice (the host baseline), the results
compared.  The library exports no sort-only entry point, so the floor of two sorts is not timed here: the --no-umi call, which is the
barcode sort, one (cell, ec) sort and the fold, stands next to the full call instead.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
T, H, CELLS, SAMPLE = 80_000, 8, 5000, 200_000


def ec_structure():
    """(lines, n_base): the distinct target sets of SAMPLE config-4 reads, then a wider copy (one foreign target more) of each."""
    from alntools_amd import synth
    g = synth.generate(synth.SynthSpec(SAMPLE, T, H, paired=True), 0, SAMPLE)
    rid = np.asarray(g["read_id"]).astype(np.int64)
    tgt = np.asarray(g["locus"]).astype(np.int64) % T * H + (np.asarray(g["hapflag"]).astype(np.int64) >> 16) % H
    pairs = np.unique(rid << 32 | tgt)
    r, t = pairs >> 32, pairs & 0xFFFFFFFF
    cut = np.flatnonzero(np.diff(r)) + 1
    sets = sorted(set(tuple(x.tolist()) for x in np.split(t, cut)))
    rng = np.random.default_rng(4)
    wide = []
    for s in sets:
        f = int(rng.integers(T * H))
        while f in s:
            f = int(rng.integers(T * H))
        wide.append(tuple(sorted(s + (f,))))
    return [list(s) for s in sets] + [list(s) for s in wide], len(sets)


def make_records(n, n_base, seed=20260101):
    import bus_checker as bc
    rng = np.random.default_rng(seed)
    m = int(n / 1.1)
    w = np.exp(rng.standard_normal(CELLS))
    cell = np.minimum(np.searchsorted(np.cumsum(w) / w.sum(), rng.random(m)), CELLS - 1)
    order = np.argsort(cell, kind="stable")
    first = np.searchsorted(cell[order], np.arange(CELLS))
    umi = np.empty(m, dtype=np.int64)
    umi[order] = np.arange(m) - first[cell[order]]                  # a UMI of its own within the cell
    barcode = (rng.permutation(1 << 24)[:CELLS].astype(np.uint64) * np.uint64(251) + np.uint64(3))[cell]
    ec = rng.integers(0, n_base, size=m)
    second = np.flatnonzero(rng.random(m) < (n - m) / m)
    ec2 = np.where(rng.random(len(second)) < 0.5, ec[second] + n_base, rng.integers(0, n_base, size=len(second)))
    bcs, umis, ecs = np.concatenate((barcode, barcode[second])), np.concatenate((umi, umi[second])), np.concatenate((ec, ec2))
    p = rng.permutation(len(bcs))
    return bc.records(bcs[p], umis[p].astype(np.uint64), ecs[p], 1)


def _timed(f, n=5):
    import torch
    wall, ev = [], []
    for _ in range(n):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = time.perf_counter()
        a.record()
        f()
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t) * 1e3)
        ev.append(a.elapsed_time(b))
    return wall, ev


def main(n):
    import torch
    import bus_checker as bc
    from alntools_amd import ecb_bus
    fmt = lambda ts: " / ".join("%.1f" % t for t in ts)   # noqa: E731
    t0 = time.perf_counter()
    lines, n_base = ec_structure()
    ptr, ids = bc.csr_lines(lines)
    tcol, thap = (np.arange(T * H) // H).astype(np.uint32), (np.arange(T * H) % H).astype(np.uint32)
    print("matrix.ec: %d lines (%d from %d config-4 reads, as many wider copies), %d target ids, longest %d; made in %.1f s"
          % (len(lines), n_base, SAMPLE, len(ids), int(np.diff(ptr.astype(np.int64)).max()), time.perf_counter() - t0), flush=True)
    t0 = time.perf_counter()
    rec = make_records(n, n_base)
    print("records: %d (%.2f GB), %d cells; made in %.1f s" % (len(rec), rec.nbytes / 1e9, CELLS, time.perf_counter() - t0), flush=True)
    for name, part in (("1/100 slice", rec[:len(rec) // 100]), ("all", rec)):
        caps = (len(part), len(part), ecb_bus.a_capacity(part, ptr), len(part))
        dev = torch.from_numpy(np.ascontiguousarray(part)).cuda()
        args = (dev, 16, 12, torch.from_numpy(ptr.view(np.int32)).cuda(), torch.from_numpy(ids.view(np.int32)).cuda(), torch.from_numpy(tcol.view(np.int32)).cuda(),
                torch.from_numpy(thap.view(np.int32)).cuda(), T, H)
        for no_umi in (False, True):
            out = ecb_bus.molecules(*args, no_umi=no_umi, capacities=caps)           # (warm-up: the pool grows here)
            sizes = out[4]
            wall, ev = _timed(lambda: ecb_bus.molecules(*args, no_umi=no_umi, capacities=caps))
            print("%s, %s: sizes (cells, rows, nnz_a, nnz_n, molecules, several ECs, discarded, new rows) %r" % (name, "--no-umi" if no_umi else "UMIs", sizes))
            print("  ecb_bus_molecules_device  wall ms: %s   HIP events ms: %s   (min %.1f ms: %.2f ns per record)"
                  % (fmt(wall), fmt(ev), min(ev), min(ev) * 1e6 / len(part)), flush=True)
            if name != "all":
                t1 = time.perf_counter()
                want = bc.molecules(part, lines, tcol, thap, no_umi=no_umi)
                t2 = time.perf_counter()
                same = (want.sizes == sizes and out[0].cpu().numpy().view(np.uint64).tolist() == want.barcodes
                        and all(np.array_equal(g.cpu().numpy(), e) for g, e in zip(out[1] + out[2], bc.csr(want.rows) + bc.csc(want.N, len(want.barcodes)))))
                print("  tests/bus_checker.py on the host: %.2f s; equal: %s" % (t2 - t1, same), flush=True)
        del dev, args, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000)
