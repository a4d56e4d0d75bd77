# -*- coding: utf-8 -*-
"""Input and timing of profiles/ecboot_c3.txt: config 3's table (the ``c3.bin`` of ``python tools/quant_c3.py write DIR``: 3.7 M ECs, 13 M
non-zeros, 80 000 loci, 8 haplotypes) with an N of one column whose W = 100 M reads are spread over the ECs in proportion to the file's own
counts (numpy's multinomial, seed 4), B = 32 replicates, seed 0.

    python tools/boot_c3.py time DIR [B]        in one process, on device arrays, wall time of each call with its waits -- two warm-up calls,
                                                then five timed ones, all listed with their minimum and median: ecb_resample_device (count-only,
                                                and filling arrays that fit), then on the same resampled N ecb_cell_support_device and
                                                ecb_quantify_cells_device at max_iters = 100 (code this feature did not touch), then
                                                ecb_quantify_bootstrap_device at max_iters = 100, with and without reps
    python tools/boot_c3.py one DIR resample|boot [B]   one such call (after one warm-up of the library's pool: an ecb_quantify_device of 0 steps),
                                                for a kernel trace of its own
"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
W, SEED, ITERS = 100 * 1000 * 1000, 0, 100


def _input(d):
    """(m, A on the device, the one-column N of W reads on the device)."""
    import torch
    from alntools_amd import bin_utils
    m = bin_utils.ecload(os.path.join(d, "c3.bin"))
    w = np.asarray(m.dataN, dtype=np.float64)
    cnt = np.random.default_rng(4).multinomial(W, w / w.sum()).astype(np.int32)
    E = m.num_reads
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()   # noqa: E731
    A = [dev(a) for a in (m.indptrA, m.indicesA, m.dataA)]
    N = [dev(a) for a in (np.array([0, E]), np.arange(E), cnt)]
    print("config 3: %d ECs, %d non-zeros, %d loci, %d haplotypes; W = %d over %d rows with weight, the heaviest %d"
          % (E, len(m.indicesA), m.num_loci, m.num_haplotypes, int(cnt.sum()), int((cnt > 0).sum()), int(cnt.max())))
    return m, A, N


def _wall(f, n=5, warm=2):
    import torch
    out = []
    for k in range(warm + n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        f()
        torch.cuda.synchronize()
        if k >= warm:
            out.append((time.perf_counter() - t) * 1e3)
    return out


def _show(what, ts):
    print("%s  ms: %s   (min %.3f, median %.3f)" % (what, " / ".join("%.3f" % t for t in ts), min(ts), float(np.median(ts))))
    return min(ts)


def _resample_call(lib, E, N, B, ptr, ec, cnt, cap):
    from alntools_amd import ecb
    p = ecb._dev_ptr
    n = C.c_uint64()
    rc = lib.ecb_resample_device(0, E, 1, E, p(N[0]), p(N[1]), p(N[2]), -1, SEED, 0, B, p(ptr), p(ec), p(cnt), cap, C.byref(n))
    assert rc == 0, lib.ecb_last_error(None)
    return n.value


def timed(d, B):
    import torch
    from alntools_amd import ecb, ecb_boot
    m, A, N = _input(d)
    T, H, E = m.num_loci, m.num_haplotypes, m.num_reads
    lib = ecb_boot.load()
    ptr = torch.empty(B + 1, dtype=torch.int32, device="cuda")
    nnz = _resample_call(lib, E, N, B, ptr, None, None, 0)
    ec, cnt = torch.empty(nnz, dtype=torch.int32, device="cuda"), torch.empty(nnz, dtype=torch.int32, device="cuda")
    print("B = %d replicates, %d draws, %d entries (%.1f %% of B x E)" % (B, B * W, nnz, 100.0 * nnz / (B * E)))
    t_count = _show("ecb_resample_device, count-only (the draws, the flags, the scan)", _wall(lambda: _resample_call(lib, E, N, B, ptr, None, None, 0)))
    t_fill = _show("ecb_resample_device, filling arrays that fit (and the emit, two allocations, two copies)",
                   _wall(lambda: _resample_call(lib, E, N, B, ptr, ec, cnt, nnz)))
    print("    %.2f G draws per second over the whole filling call" % (B * W / t_fill / 1e6))
    rep = (ptr, ec, cnt)
    ns = int(ecb.cell_support(*A, T, H, *rep, count_only=True)[0][-1])
    t_sup = _show("beside it: ecb_cell_support_device on the resampled N (count-only)", _wall(lambda: ecb.cell_support(*A, T, H, *rep, count_only=True), 3, 1))
    info = ecb.quantify_cells(*A, T, H, *rep, max_iters=ITERS, n_slots=ns)[3]
    it = info["n_iter"].cpu().numpy()
    print("    %d slots; steps per replicate at max_iters = %d, tol 1e-6: %d .. %d, %d converged" % (ns, ITERS, it.min(), it.max(), int(info["converged"].sum())))
    t_em = _show("beside it: ecb_quantify_cells_device on the resampled N, max_iters = %d (n_slots known)" % ITERS,
                 _wall(lambda: ecb.quantify_cells(*A, T, H, *rep, max_iters=ITERS, n_slots=ns), 3, 0))
    boot = lambda reps: ecb_boot.quantify_bootstrap(*A, T, H, *N, n_reps=B, seed=SEED, max_iters=ITERS, return_reps=reps)   # noqa: E731
    t_boot = _show("ecb_quantify_bootstrap_device, max_iters = %d, without reps" % ITERS, _wall(lambda: boot(False), 3, 1))
    _show("ecb_quantify_bootstrap_device, max_iters = %d, with reps" % ITERS, _wall(lambda: boot(True), 3, 0))
    print("drawing and compacting %d replicates: %.1f ms; quantifying them (support + EM): %.1f ms; ratio %.3f; the bootstrap call %.1f ms"
          % (B, t_fill, t_sup + t_em, t_fill / (t_sup + t_em), t_boot))
    res = boot(True)
    cp, sl, th, _ = ecb.quantify_cells(*A, T, H, *rep, max_iters=ITERS, n_slots=ns)
    import boot_checker
    want = boot_checker.scatter(cp.cpu().numpy(), sl.cpu().numpy(), th.cpu().numpy(), T, H)
    print("reps equal ecb.quantify_cells on the resampled N, scattered: %s" % (res[5].cpu().numpy().tobytes() == want.tobytes()))
    mean, sd = res[0].cpu().numpy(), res[1].cpu().numpy()
    live = mean > 1.0
    print("sum of mean %.3f (W = %d); median sd / mean over the %d entries with mean > 1: %.4f" % (mean.sum(), W, live.sum(), np.median(sd[live] / mean[live])))


def one(d, which, B):
    import torch
    from alntools_amd import ecb, ecb_boot
    m, A, N = _input(d)
    T, H, E = m.num_loci, m.num_haplotypes, m.num_reads
    ecb.quantify(*A, T, H, *N, max_iters=0)
    torch.cuda.synchronize()
    if which == "resample":
        out = ecb_boot.resample(E, *N, seed=SEED, n_reps=B)
        print("entries", len(out[1]))
    else:
        print(ecb_boot.quantify_bootstrap(*A, T, H, *N, n_reps=B, seed=SEED, max_iters=ITERS)[4]["n_iter"])
    torch.cuda.synchronize()


if __name__ == "__main__":
    if sys.argv[1] == "one":
        one(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 32)
    else:
        timed(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 32)
