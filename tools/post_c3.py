# -*- coding: utf-8 -*-
"""Timing of profiles/ecposterior_c3.txt: ``ecb_posterior_device`` for models 4 and 1-3 and ``ecb_csr_to_hapcsc_values_device`` at config 3's
size and gene partition (the ``c3.bin`` and ``c3.grp.txt`` of ``tools/quant_c3.py write DIR``: 3.7 M ECs, 13 M non-zeros, 80 000 loci, 8
haplotypes), beside what the code the feature did not touch measures in the same process: one EM step of the same model (the wall time of
40 steps less that of 8, over 32) and ``ecb_csr_to_hapcsc_device``.

    python tools/quant_c3.py write DIR      the files
    python tools/post_c3.py time DIR        in one process: two warm-up calls, then seven timed calls of each, wall time of the call on device
                                            arrays with its waits (ms: all seven, the minimum and the median); the flat posterior's traffic
                                            -- A read once, 8 bytes gathered and 8 written per set bit -- against the copy rate
                                            ``bench.py --full`` measures (``bench.copy_peak``), on the same device; and the results
                                            checked: one row per model against ``tests/post_checker.py``, the payload as a permutation
    python tools/post_c3.py one DIR MODEL   ecb_posterior_device once (MODEL 1..4), or ``values``: the transposition once (for a kernel trace)
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

REPS, WARM = 7, 2


def _wall(f, n=REPS, warm=WARM):
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


def _fmt(ts):
    return "%s   (min %.3f, median %.3f)" % (" / ".join("%.3f" % t for t in ts), min(ts), float(np.median(ts)))


def _setup(d):
    import torch
    from alntools_amd import bin_utils
    m = bin_utils.ecload(os.path.join(d, "c3.bin"))
    gene, names = bin_utils.gene_ids(m, os.path.join(d, "c3.grp.txt"))
    dev = lambda arrays: [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda() for a in arrays]      # noqa: E731
    return m, dev((m.indptrA, m.indicesA, m.dataA)), dev((m.indptrN, m.indicesN, m.dataN)), torch.from_numpy(gene).cuda(), gene, len(names)


def one(d, which):
    import torch
    from alntools_amd import ecb
    m, A, N, gene, _, G = _setup(d)
    T, H = m.num_loci, m.num_haplotypes
    theta = ecb.quantify(*A, T, H, *N, max_iters=0)[0]
    torch.cuda.synchronize()
    if which == "values":
        post = ecb.posterior(*A, T, H, theta)[0]
        ecb.csr_to_hapcsc_values(*A, post, T, H)
    else:
        ecb.posterior(*A, T, H, theta, gene=gene, n_genes=G, model=int(which))
    torch.cuda.synchronize()


def timed(d):
    import torch
    import bench
    import post_checker as pchk
    import quant_checker as qchk
    import quant_model_checker as mchk
    from alntools_amd import ecb
    m, A, N, gene, gene_h, G = _setup(d)
    T, H = m.num_loci, m.num_haplotypes
    E, nnz = m.num_reads, len(m.indicesA)
    theta = ecb.quantify(*A, T, H, *N, max_iters=3, tol=0.0)[0]
    post, bit_ptr, mass = ecb.posterior(*A, T, H, theta)
    n_bits = post.numel()
    print("config 3: %d ECs, %d non-zeros, %d set bits, %d loci, %d haplotypes, %d genes" % (E, nnz, n_bits, T, H, G))
    steps = {4: lambda k: ecb.quantify(*A, T, H, *N, max_iters=k, tol=0.0)}
    for mo in (1, 2, 3):
        steps[mo] = lambda k, mo=mo: ecb.quantify_model(*A, T, H, *N, gene, G, mo, max_iters=k, tol=0.0)
    mins = {}
    for mo in (4, 1, 2, 3):
        w = _wall(lambda: ecb.posterior(*A, T, H, theta, gene=gene, n_genes=G, model=mo))
        w8, w40 = _wall(lambda: steps[mo](8), 5, 1), _wall(lambda: steps[mo](40), 5, 1)
        w0 = _wall(lambda: steps[mo](0), 5, 1)
        mins[mo] = min(w)
        print("ecb.posterior (the wrapper: the count-only conversion call, three allocations, then ecb_posterior_device), model %d  ms: %s" % (mo, _fmt(w)))
        print("    beside it: the EM of model %d, set-up (0 steps) %.3f ms, one step (40 against 8 steps, the minima) %.1f us"
              % (mo, min(w0), (min(w40) - min(w8)) / 32 * 1e3))
    tv = _wall(lambda: ecb.csr_to_hapcsc_values(*A, post, T, H))
    ti = _wall(lambda: ecb.csr_to_hapcsc(*A, T, H))
    print("ecb.csr_to_hapcsc_values (count-only call, three allocations, ecb_csr_to_hapcsc_values_device)  ms: %s" % _fmt(tv))
    print("ecb.csr_to_hapcsc        (two allocations, ecb_csr_to_hapcsc_device)                             ms: %s" % _fmt(ti))
    # the entry point itself: outputs allocated once, n_bits known
    lib = ecb.load()
    outs = (torch.empty(n_bits, dtype=torch.float64, device="cuda"), torch.empty(nnz + 1, dtype=torch.int64, device="cuda"),
            torch.empty(E, dtype=torch.float64, device="cuda"))
    th = theta.contiguous()

    def raw(mo, with_opt=True):
        rc = lib.ecb_posterior_device(0, E, T, H, nnz, ecb._dev_ptr(A[0]), ecb._dev_ptr(A[1]), ecb._dev_ptr(A[2]), None, ecb._dev_ptr(th), G,
                                      ecb._dev_ptr(gene), mo, n_bits, ecb._dev_ptr(outs[0]), ecb._dev_ptr(outs[1]) if with_opt else None,
                                      ecb._dev_ptr(outs[2]) if with_opt else None)
        assert rc == 0, lib.ecb_last_error(None)
    raw_min = {}
    for mo in (4, 1, 2, 3):
        w = _wall(lambda: raw(mo))
        raw_min[mo] = min(w)
        print("ecb_posterior_device (outputs allocated once, n_bits known), model %d  ms: %s" % (mo, _fmt(w)))
    w = _wall(lambda: raw(4, False))
    print("    model 4 without bit_ptr and row_mass  ms: %s" % _fmt(w))
    import ctypes as C
    cp_o, ci_o = torch.empty((H, T + 1), dtype=torch.int32, device="cuda"), torch.empty(n_bits, dtype=torch.int32, device="cuda")
    cd_o, tot = torch.empty(n_bits, dtype=torch.float64, device="cuda"), C.c_uint64()
    head = (0, E, T, H, ecb._dev_ptr(A[0]), ecb._dev_ptr(A[1]), ecb._dev_ptr(A[2]))

    def raw_values():
        assert lib.ecb_csr_to_hapcsc_values_device(*head, ecb._dev_ptr(post), ecb._dev_ptr(cp_o), ecb._dev_ptr(ci_o), ecb._dev_ptr(cd_o), C.byref(tot)) == 0

    def raw_incidence():
        assert lib.ecb_csr_to_hapcsc_device(*head, ecb._dev_ptr(cp_o), ecb._dev_ptr(ci_o), C.byref(tot)) == 0
    print("ecb_csr_to_hapcsc_values_device (outputs allocated once)  ms: %s" % _fmt(_wall(raw_values)))
    print("ecb_csr_to_hapcsc_device        (outputs allocated once)  ms: %s" % _fmt(_wall(raw_incidence)))
    copy, read, how = bench.copy_peak(torch.device("cuda:0"))
    traffic = (E + 1) * 4 + nnz * 8 + n_bits * 16
    print("the flat posterior moves %.1f MB (A once, 8 bytes gathered and 8 written per set bit): %.0f GB/s over the whole call's %.3f ms;"
          % (traffic / 1e6, traffic / (raw_min[4] * 1e-3) / 1e9, raw_min[4]))
    print("    the copy rate of this device: %.0f GB/s (%s)" % (copy, how))
    # the results: model 4's values of a few rows against the checker's, the weighted sum against one step, the payload a permutation
    p = qchk.Problem(m.indptrA, m.indicesA, m.dataA, T, H, m.indptrN, m.indicesN, m.dataN)
    lay = pchk.Layout.of(m)
    q = mchk.Grouping(p, gene_h, G)
    th_h = theta.cpu().numpy()
    for mo in (4, 1, 2, 3):
        got = ecb.posterior(*A, T, H, theta, gene=gene, n_genes=G, model=mo)[0].cpu().numpy()
        ref = pchk.posterior(q, lay, mo, th_h)[0]
        bound = pchk.tolerance(mo, p.B, H, q.M, q.R)
        print("model %d equals tests/post_checker.py's within %.3g (bound %.3g)" % (mo, qchk.agree(got, ref, bound), bound))
    cp, ci, cd = ecb.csr_to_hapcsc_values(*A, torch.arange(n_bits, dtype=torch.float64, device="cuda"), T, H)
    cp0, ci0 = ecb.csr_to_hapcsc(*A, T, H)
    assert torch.equal(cp, cp0) and torch.equal(ci, ci0)
    assert np.array_equal(cd.cpu().numpy(), lay.csc_to_bit.astype(np.float64))
    print("the transposition's indptr and indices are ecb_csr_to_hapcsc_device's, its data the checker's permutation of 0 .. n_bits - 1")


if __name__ == "__main__":
    if sys.argv[1] == "one":
        one(sys.argv[2], sys.argv[3])
    else:
        timed(sys.argv[2])
