# -*- coding: utf-8 -*-
"""Input and timing of profiles/bus_correct_c4.txt: ``tools/bus_c4.py``'s synthetic BUS file (100 M records, 5 000 cells) with 5 % of its
records' barcodes changed in one base and 1 % in two, against a whitelist of 6.8 M random 16-base barcodes that holds the cells'.

    python tools/bus_correct_c4.py [N_RECORDS]       (default 100 000 000)

Reports, from one process: the wall time and the HIP-event time of ``ecb_bus_correct_device`` on device arrays, warm, five calls; a
device-to-device copy of the same records (the floor of the emit pass: every kept record is read once and written once); the warm
``ecb_bus_molecules_device`` call that the corrected records feed; and the call on a 1/500 slice next to
``tests/bus_correct_checker.py`` on that slice, the results compared.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
N_WHITE = 6_800_000


def damage(rec, seed=7):
    """5 % of the records with one base of the barcode changed, another 1 % with two (in place)."""
    rng = np.random.default_rng(seed)
    bcs = rec.reshape(-1).view("<u8")[::4]                              # (the barcode is the first of a record's four 8-byte words)
    n = len(bcs)
    u = rng.random(n)
    for share_lo, share_hi, times in ((0.0, 0.05, 1), (0.05, 0.06, 2)):
        at = np.flatnonzero((u >= share_lo) & (u < share_hi))
        pos = rng.integers(0, 16, size=len(at))
        for k in range(times):
            p = (pos + 5 * k) % 16                                      # (two different positions)
            bcs[at] ^= rng.integers(1, 4, size=len(at)).astype(np.uint64) << (2 * p).astype(np.uint64)
    return rec


def main(n):
    import torch
    import bus_c4
    import bus_checker as bc
    import bus_correct_checker as cc
    from alntools_amd import ecb_bus, ecb_bus_correct as ebc
    fmt = lambda ts: " / ".join("%.2f" % t for t in ts)   # noqa: E731
    lines, n_base = bus_c4.ec_structure()
    ptr, ids = bc.csr_lines(lines)
    T, H = bus_c4.T, bus_c4.H
    tcol, thap = (np.arange(T * H) // H).astype(np.uint32), (np.arange(T * H) % H).astype(np.uint32)
    t0 = time.perf_counter()
    rec = bus_c4.make_records(n, n_base)
    cells = np.unique(rec.reshape(-1).view("<u8")[::4])
    rng = np.random.default_rng(68)
    white = np.unique(np.concatenate((cells, rng.integers(0, 1 << 32, size=N_WHITE - len(cells), dtype=np.uint64))))
    rec = damage(rec)
    print("records: %d (%.2f GB), %d cells, 5 %% one base off, 1 %% two; whitelist: %d entries (%.1f MB); made in %.1f s"
          % (len(rec), rec.nbytes / 1e9, len(cells), len(white), white.nbytes / 1e6, time.perf_counter() - t0), flush=True)
    d_white = torch.from_numpy(white.view(np.int64)).cuda()
    for name, part in (("1/500 slice", rec[:len(rec) // 500]), ("all", rec)):
        dev = torch.from_numpy(np.ascontiguousarray(part)).cuda()
        out, status, sizes = ebc.correct(dev, 16, d_white, want_status=True)           # (warm-up: the pool grows here)
        wall, ev = bus_c4._timed(lambda: ebc.correct(dev, 16, d_white, want_status=True))
        print("%s: sizes (exact, corrected, without a candidate, ambiguous) %r" % (name, sizes))
        print("  ecb_bus_correct_device  wall ms: %s   HIP events ms: %s   (min %.2f ms: %.3f ns per record, %.1f ns per miss)"
              % (fmt(wall), fmt(ev), min(ev), min(ev) * 1e6 / len(part), min(ev) * 1e6 / max(sum(sizes[1:]), 1)), flush=True)
        wall, ev = bus_c4._timed(lambda: ebc.correct(dev, 16, d_white, want_status=False))
        print("  ... without the status bytes  HIP events ms: %s" % fmt(ev), flush=True)
        if name != "all":
            t1 = time.perf_counter()
            want = cc.correct(part, 16, white)
            t2 = time.perf_counter()
            same = want[2] == sizes and np.array_equal(out.cpu().numpy(), want[1]) and np.array_equal(status.cpu().numpy(), want[0])
            print("  tests/bus_correct_checker.py on the host: %.2f s; equal: %s" % (t2 - t1, same), flush=True)
            continue
        dst = torch.empty_like(dev)
        wall, ev = bus_c4._timed(lambda: dst.copy_(dev))
        print("  device-to-device copy of the records (%.2f GB read, as much written)  HIP events ms: %s   (min %.2f ms)"
              % (dev.numel() / 1e9, fmt(ev), min(ev)), flush=True)
        del dst
        kept = out.contiguous()
        caps = (len(kept), len(kept), ecb_bus.a_capacity(kept.cpu().numpy(), ptr), len(kept))
        args = (kept, 16, 12, torch.from_numpy(ptr.view(np.int32)).cuda(), torch.from_numpy(ids.view(np.int32)).cuda(), torch.from_numpy(tcol.view(np.int32)).cuda(),
                torch.from_numpy(thap.view(np.int32)).cuda(), T, H)
        res = ecb_bus.molecules(*args, capacities=caps)
        wall, ev = bus_c4._timed(lambda: ecb_bus.molecules(*args, capacities=caps), n=3)
        print("  ecb_bus_molecules_device on the %d records kept: %d cells   HIP events ms: %s   (min %.1f ms)" % (len(kept), res[4][0], fmt(ev), min(ev)), flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000)
