# -*- coding: utf-8 -*-
"""Input and timing of profiles/ecselect_c4.txt: a synthetic config-4-shaped ``.bin`` built on the device (3 M ECs of 1 - 7 loci over 80 000
targets, 2 haplotypes; 5 000 samples of 10 000 - 30 000 entries of N each, ~10^8 in all, ascending within a column, seed 4) run through
``ecb_select_device``.

    python tools/select_c4.py time           the small cases checked against tests/select_checker.py first; then, warm, the wall time of
                                             the call (waits and its two read-backs included) for: a threshold alone (the median total:
                                             half the samples leave), --unique alone, --multi with a threshold; the bytes each must move
                                             (every input once, every output once) and that as a fraction of the copy rate measured here
    python tools/select_c4.py one NAME       one call of the variant NAME (threshold, unique, multi_threshold), for a kernel trace of its own
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

E, T, H, S = 3000000, 80000, 2, 5000


def inputs(seed=4, device="cuda", sizes=(10000, 30001)):
    """The six arrays on ``device`` (tools/quant_c4.py rehearses on the CPU at a toy size)."""
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    i32 = torch.int32
    lens = torch.randint(1, 8, (E,), generator=g, device=device)
    ipa = torch.zeros(E + 1, dtype=torch.int64, device=device)
    ipa[1:] = torch.cumsum(lens, 0)
    row = torch.repeat_interleave(torch.arange(E, device=device), lens)
    start = torch.randint(0, T - 8, (E,), generator=g, device=device)
    ixa = torch.arange(int(ipa[-1]), device=device) - ipa[:-1][row] + start[row]
    daa = torch.randint(1, 1 << H, (int(ipa[-1]),), generator=g, device=device)
    daa[torch.rand(len(daa), generator=g, device=device) < 0.5] = 1          # half the non-zeros carry one haplotype
    sizes = torch.randint(sizes[0], sizes[1], (S,), generator=g, device=device)
    ipn = torch.zeros(S + 1, dtype=torch.int64, device=device)
    ipn[1:] = torch.cumsum(sizes, 0)
    n = int(ipn[-1])
    col = torch.repeat_interleave(torch.arange(S, device=device), sizes)
    key, _ = torch.sort(col * E + torch.randint(0, E, (n,), generator=g, device=device))
    ixn = key - col * E
    dan = torch.randint(1, 20, (n,), generator=g, device=device)
    del key, col, row
    out = [x.to(i32).contiguous() for x in (ipa, ixa, daa, ipn, ixn, dan)]
    if device == "cuda":
        torch.cuda.synchronize()
    return out


def variants(a):
    """name -> (row_class, min_count): the threshold is the median of the samples' totals over the rows in class."""
    import torch
    from alntools_amd import ecb
    out = {}
    for name, row_class, thresholded in (("threshold", None, True), ("unique", "unique", False), ("multi_threshold", "multi", True)):
        mc = None
        if thresholded:
            (_, _, _, ipn, ixn, dan), _ = ecb.select(*a, T, H, row_class=row_class)          # N over the rows in class, all samples
            tot = torch.zeros(S, dtype=torch.int64, device="cuda")
            tot.index_add_(0, torch.repeat_interleave(torch.arange(S, device="cuda"), (ipn[1:] - ipn[:-1]).long()), dan.long())
            mc = int(tot.median())
        out[name] = (row_class, mc)
    return out


def copy_rate():
    """GB/s of a device-to-device copy of 1 GiB (read + write), the best of five."""
    import torch
    src = torch.empty(1 << 28, dtype=torch.int32, device="cuda").fill_(1)
    dst = torch.empty_like(src)
    best = 1e9
    for _ in range(6):
        torch.cuda.synchronize()
        t = time.perf_counter()
        dst.copy_(src)
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return 2 * src.numel() * 4 / best / 1e9


def check_small():
    import select_checker
    import test_gpu_ecselect as tg
    ok = True
    for Hs, Ss in ((2, 3), (8, 338)):
        m, keep, _ = tg._random(100 * Hs + Ss, Hs, Ss)
        for row_class in select_checker.CLASSES:
            for mc in (None, 40):
                exp = select_checker.select_flags(m, row_class, keep, mc)[0]
                got = tg._device(m, row_class, keep, mc, tensors=True)[0]
                ok &= tg.bin_utils.ecsave2_bytes(got) == tg.bin_utils.ecsave2_bytes(exp)
    print("small cases equal tests/select_checker.py:", ok)


def timed():
    import torch
    from alntools_amd import ecb
    check_small()
    a = inputs()
    nnz_a, nnz_n = len(a[1]), len(a[4])
    print("config-4 shape: %d ECs, %d non-zeros of A, %d samples, %d entries of N" % (E, nnz_a, S, nnz_n))
    rate = copy_rate()
    print("device-to-device copy of 1 GiB: %.0f GB/s (read + write)" % rate)
    for name, (row_class, mc) in variants(a).items():
        ts = []
        for _ in range(6):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out, kept = ecb.select(*a, T, H, row_class=row_class, min_count=mc)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t) * 1e3)
        ts = ts[1:]
        moved = 4 * (E + 1 + 2 * nnz_a + S + 1 + 2 * nnz_n) + 4 * sum(len(o) for o in out) + S
        gbs = moved / (min(ts) * 1e-3) / 1e9
        print("%-16s class %-6s -m %-8s ms: %s   (min %.2f)   -> %d ECs, %d non-zeros, %d samples, %d entries;  %.2f GB to move: %.0f GB/s, %.2f of the copy rate"
              % (name, row_class or "all", mc, " / ".join("%.2f" % t for t in ts), min(ts), len(out[0]) - 1, len(out[1]), int(kept.sum()), len(out[4]),
                 moved / 1e9, gbs, gbs / rate))


if __name__ == "__main__":
    if sys.argv[1] == "one":
        import torch
        from alntools_amd import ecb
        a = inputs()
        rc, mc = variants(a)[sys.argv[2]]
        ecb.select(*a, T, H, row_class=rc, min_count=mc)
        ecb.select(*a, T, H, row_class=rc, min_count=mc)
        torch.cuda.synchronize()
    else:
        timed()
