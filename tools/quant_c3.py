# -*- coding: utf-8 -*-
"""Input and timing of profiles/ecquant_c3.txt: the config-3-sized ``.bin`` of ``tests/gt_checker.py:write_c3_files`` (3.7 M ECs,
13 M non-zeros, 80 000 loci, 8 haplotypes, seed 3), the one ``tools/count_c3.py`` writes.

    python tools/quant_c3.py write DIR            the files
    python tools/quant_c3.py one DIR quant [K]    ecb_quantify_device once on device arrays, K steps (default 20), tol 0 (for a kernel trace of its own)
    python tools/quant_c3.py one DIR transpose    ecb_csr_to_hapcsc_device once on the same arrays: the yardstick, code the feature did not touch
    python tools/quant_c3.py one DIR models [K]   the flat step and then models 1, 2 and 3 over DIR/c3.grp.txt, one call each on device arrays,
                                                  K steps, tol 0 (for a kernel trace of its own: profiles/ecquant_models_c3.txt)
    python tools/quant_c3.py models DIR           in one process, warm, wall time of the flat call and of each model's with 8 and 40 steps
    python tools/quant_c3.py time DIR             in one process, warm, wall time of the call with its waits: ecb_quantify_device with 0, 1, 8 and
                                                  40 steps (the set-up and the time per step are their differences), ecb_csr_to_hapcsc_device,
                                                  the numpy checker's step, and one device step checked against the checker's
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _load(d):
    from alntools_amd import bin_utils
    return bin_utils.ecload(os.path.join(d, "c3.bin"))


def _dev(arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda() for a in arrays]


def one(d, which, steps=20):
    import torch
    from alntools_amd import ecb
    m = _load(d)
    A, N = _dev((m.indptrA, m.indicesA, m.dataA)), _dev((m.indptrN, m.indicesN, m.dataN))
    torch.cuda.synchronize()
    if which == "quant":
        print(ecb.quantify(*A, m.num_loci, m.num_haplotypes, *N, max_iters=steps, tol=0.0)[1])
    elif which == "models":
        gene, names = _genes(d, m)
        print("flat", ecb.quantify(*A, m.num_loci, m.num_haplotypes, *N, max_iters=steps, tol=0.0)[1])
        for model in (1, 2, 3):
            print("model", model, ecb.quantify_model(*A, m.num_loci, m.num_haplotypes, *N, gene, len(names), model, max_iters=steps, tol=0.0)[1])
    else:
        ecb.csr_to_hapcsc(*A, m.num_loci, m.num_haplotypes)
    torch.cuda.synchronize()


def _genes(d, m):
    """(gene[t] on the device, the genes' names) of DIR/c3.grp.txt."""
    import torch
    from alntools_amd import bin_utils
    gene, names = bin_utils.gene_ids(m, os.path.join(d, "c3.grp.txt"))
    members = np.bincount(gene)
    print("%d genes, the largest with %d members, %d with more than one" % (len(names), members.max(), (members > 1).sum()))
    return torch.from_numpy(gene).cuda(), names


def _wall(f, n=5):
    import torch
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        f()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def timed(d):
    import quant_checker
    from alntools_amd import ecb
    m = _load(d)
    T, H = m.num_loci, m.num_haplotypes
    host = (m.indptrA, m.indicesA, m.dataA)
    Nh = (m.indptrN, m.indicesN, m.dataN)
    A, N = _dev(host), _dev(Nh)
    p = quant_checker.Problem(*host, T, H, *Nh)
    print("config 3: %d ECs, %d non-zeros, %d set bits, B = %d, L = %d" % (p.E, p.nnz, len(p.bit_row), p.B, p.L))
    t0 = time.perf_counter()
    ref, explained = quant_checker.step(p, p.aln())
    t_chk = (time.perf_counter() - t0) * 1e3
    got, info = ecb.quantify(*A, T, H, *N, max_iters=1, tol=0.0)
    worst = quant_checker.agree(got.cpu().numpy(), ref, p.tolerance())
    print("one step equals tests/quant_checker.py's within %.3g (bound %.3g); explained %d = %d" % (worst, p.tolerance(), info["explained"], explained))
    ecb.csr_to_hapcsc(*A, T, H)
    fmt = lambda ts: " / ".join("%.3f" % t for t in ts)   # noqa: E731
    mins = {}
    for k in (0, 1, 8, 40):
        w = _wall(lambda: ecb.quantify(*A, T, H, *N, max_iters=k, tol=0.0))
        mins[k] = min(w)
        print("ecb_quantify_device, %2d steps  ms: %s   (min %.3f)" % (k, fmt(w), min(w)))
    print("set-up (0 steps) %.3f ms; per step (40 against 8 steps) %.1f us" % (mins[0], (mins[40] - mins[8]) / 32 * 1e3))
    t = _wall(lambda: ecb.csr_to_hapcsc(*A, T, H))
    print("ecb_csr_to_hapcsc_device     ms: %s   (min %.3f)" % (fmt(t), min(t)))
    print("tests/quant_checker.py step (numpy, this host's CPU)  ms: %.1f" % t_chk)
    theta, info = ecb.quantify(*A, T, H, *N, tol=1e-6)
    w = _wall(lambda: ecb.quantify(*A, T, H, *N, tol=1e-6), 3)
    print("to tol 1e-6: %s  ms: %s" % (info, fmt(w)))


def models(d):
    from alntools_amd import ecb
    m = _load(d)
    T, H = m.num_loci, m.num_haplotypes
    A, N = _dev((m.indptrA, m.indicesA, m.dataA)), _dev((m.indptrN, m.indicesN, m.dataN))
    gene, names = _genes(d, m)
    fmt = lambda ts: " / ".join("%.3f" % t for t in ts)   # noqa: E731
    calls = [("flat", lambda k: ecb.quantify(*A, T, H, *N, max_iters=k, tol=0.0))]
    calls += [("model %d" % mo, lambda k, mo=mo: ecb.quantify_model(*A, T, H, *N, gene, len(names), mo, max_iters=k, tol=0.0)) for mo in (1, 2, 3)]
    for name, f in calls:
        f(1)
        mins = {}
        for k in (0, 8, 40):
            w = _wall(lambda: f(k))
            mins[k] = min(w)
            print("%s, %2d steps  ms: %s   (min %.3f)" % (name, k, fmt(w), min(w)))
        print("%s: set-up (0 steps) %.3f ms; per step (40 against 8 steps) %.1f us; sum of theta %r, explained %d"
              % (name, mins[0], (mins[40] - mins[8]) / 32 * 1e3, float(f(1)[0].sum()), f(1)[1]["explained"]))


if __name__ == "__main__":
    if sys.argv[1] == "write":
        import gt_checker
        os.makedirs(sys.argv[2], exist_ok=True)
        print(gt_checker.write_c3_files(sys.argv[2]))
    elif sys.argv[1] == "one":
        one(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 20)
    elif sys.argv[1] == "models":
        models(sys.argv[2])
    else:
        timed(sys.argv[2])
