# -*- coding: utf-8 -*-
"""Input and timing of profiles/ecdownsample_c4.txt: ``ecb_downsample_device`` on two synthetic N of 100 M reads, thinned to half --

    cells    config 4's shape: 5 000 samples of 2 000 entries each, counts 1 .. 19 (about 20 000 reads a sample: every one on the large path)
    bulk     one sample of 1 000 000 entries, counts 1 .. 199

    python tools/downsample_c4.py time [READS]       (default 100 000 000)
    python tools/downsample_c4.py one cells|bulk|draw [READS]

``time``: from one process, per shape, the host clock around the warm call (it ends in a wait for the device), five calls, next to
``ecb_resample_device`` of ONE pooled replicate of the same N (ecboot's ``k_bs_draw``: one Philox output per read too; its call also holds
the set-up and the compaction of the replicate), and the checker's time on the host for 1 M reads.  The result is held to what can be
checked at this size without the checker: every sample keeps exactly its target, no entry more than it had.  ``one``: a single call, for a
kernel trace (``rocprofv3 --kernel-trace --stats``: the passes taken are the calls of ``k_ds_hist``).
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
N_ECS, SEED = 200_000, 7


def make(shape, reads):
    """-> (indptr, indices, counts, target) as CUDA tensors, and the reads they hold."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(4)
    if shape == "cells":
        S, per, top = 5000, max(1, reads // (5000 * 10)), 20
    else:
        S, per, top = 1, max(1, reads // 100), 200
    nnz = S * per
    cnt = torch.randint(1, top, (nnz,), generator=g, device="cuda", dtype=torch.int32)
    ec = torch.randint(0, N_ECS, (nnz,), generator=g, device="cuda", dtype=torch.int32)
    ptr = (torch.arange(S + 1, device="cuda", dtype=torch.int64) * per).to(torch.int32)
    tot = cnt.view(S, per).sum(dim=1, dtype=torch.int64)
    return ptr, ec, cnt, tot // 2, int(tot.sum())


def check(ptr, cnt, target, out, tin, tout):
    import torch
    S = len(target)
    per = len(cnt) // S
    assert torch.equal(tout, target) and torch.equal(tin, cnt.view(S, per).sum(dim=1, dtype=torch.int64))
    assert torch.equal(out.view(S, per).sum(dim=1, dtype=torch.int64), target) and bool((out >= 0).all()) and bool((out <= cnt).all())


def clock(fn, n=5):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def main():
    import torch
    from alntools_amd import ecb_boot, ecb_downsample as ed
    what = sys.argv[1] if len(sys.argv) > 1 else "time"
    if what == "one":
        shape, reads = sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 100_000_000
        ptr, ec, cnt, target, total = make("cells" if shape == "draw" else shape, reads)
        if shape == "draw":
            ecb_boot.resample(N_ECS, ptr, ec, cnt, seed=SEED, n_reps=1)
        else:
            ed.downsample(ptr, ec, cnt, N_ECS, target, seed=SEED)
        torch.cuda.synchronize()
        print("one %s: %d reads" % (shape, total))
        return
    reads = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
    for shape in ("cells", "bulk"):
        ptr, ec, cnt, target, total = make(shape, reads)
        out, tin, tout = ed.downsample(ptr, ec, cnt, N_ECS, target, seed=SEED)
        check(ptr, cnt, target, out, tin, tout)
        again = ed.downsample(ptr, ec, cnt, N_ECS, target, seed=SEED)[0]
        assert torch.equal(out, again)
        ms = clock(lambda: ed.downsample(ptr, ec, cnt, N_ECS, target, seed=SEED))
        best = min(ms)
        print("%-5s  %d samples, %d entries, %d reads -> half: ecb_downsample_device %s ms  (best %.2f ms: %.2f G reads/s)"
              % (shape, len(target), len(cnt), total, " ".join("%.2f" % m for m in ms), best, total / best / 1e6))
        if shape == "cells":
            ms = clock(lambda: ecb_boot.resample(N_ECS, ptr, ec, cnt, seed=SEED, n_reps=1))
            print("       ecb_resample_device, one pooled replicate of the same N (%d draws): %s ms  (best %.2f ms: %.2f G draws/s)"
                  % (total, " ".join("%.2f" % m for m in ms), min(ms), total / min(ms) / 1e6))
    import downsample_checker as dc
    counts = np.random.default_rng(1).integers(1, 20, 100_000)
    M = int(counts.sum())
    t0 = time.perf_counter()
    dc.thin_column(counts, 0, M // 2, SEED)
    dt = time.perf_counter() - t0
    print("checker on the host: %d reads in %.2f s (%.2f M reads/s)" % (M, dt, M / dt / 1e6))


if __name__ == "__main__":
    main()
