# -*- coding: utf-8 -*-
"""Input and timing of profiles/ecquant_cells_c4.txt: the synthetic config-4-shaped ``.bin`` of ``tools/select_c4.py`` (3 M ECs of 1 - 7 loci
over 80 000 targets, 2 haplotypes; 5 000 samples of 10 000 - 30 000 entries of N each, ~10^8 in all, seed 4) run through
``ecb_quantify_cells_device``: one EM per cell, all cells together.

    python tools/quant_c4.py time [S]        two cells checked against tests/cell_quant_checker.py first; then, warm, the wall time of the call
                                             with its waits: the support alone, 0 steps (the set-up), 8 and 24 steps (the time per step while
                                             most cells still run is their difference), the run to tol 1e-6; the step's algorithmic bytes against
                                             the HBM peak; the share of the launched work that fell on cells already done; and the yardstick, the
                                             code as it was: ecb.quantify(sample=c, tol=1e-6) on a seeded sample of 64 cells, scaled by S / 64.
                                             S: the first S samples only (default: all 5 000)
    python tools/quant_c4.py one [S] [K] [M]  one call of K steps (default 16), tol 0, for a kernel trace of its own; M: model 1, 2 or 3 over the
                                             gene map of ``models`` (default: the flat step)
    python tools/quant_c4.py models [S]      profiles/ecquant_cells_models_c4.txt: ``ecb_quantify_cells_model_device`` over a seeded gene map (T / 4
                                             genes, ids drawn per target, so a gene's members are scattered) -- per model, two cells checked against
                                             tests/cell_model_checker.py first; then, warm, in one process on one build, the flat cells step and
                                             every model's: 0 steps (the set-up), 8 and 24 steps, the time per step while every cell still runs
                                             (24 against 8 steps), and its ratio to the flat step's
    python tools/quant_c4.py rehearse        the same paths at a toy size on the CPU, the numpy checkers standing in for the device: no times
"""
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

HBM_PEAK = 8.0e12          # bytes / s


def _wall(f, n=3):
    import torch
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        f()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def _cpu_wall(f, n=3):
    """(rehearsal only: the calls are made, their times mean nothing)"""
    out = []
    for _ in range(n):
        t = time.perf_counter()
        f()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def _fmt(ts):
    return " / ".join("%.2f" % t for t in ts) + "   (median %.2f)" % float(np.median(ts))


def step_bytes(x, entries, items, slots):
    """What one step of all cells must move: E-step (slot, mask) per expanded non-zero, per entry its two offsets' worth, its count, r and
    its explained flag; M-step (entry, mask) per column element, per (slot, h) theta and phi read and written, per slot its pointer."""
    return x * 8 + entries * (4 + 4 + 8 + 1) + x * 8 + items * 32 + slots * 4


def report(a, T, H, S, E, quantify_cells, cell_support, quantify, wall, sample=64):
    ipa, ixa, daa, ipn, ixn, dan = a
    host = [np.asarray(t.cpu() if hasattr(t, "cpu") else t) for t in a]
    lens = np.diff(host[0].astype(np.int64))
    cell_of = np.repeat(np.arange(S), np.diff(host[3].astype(np.int64)))
    x_cell = np.bincount(cell_of, weights=lens[host[4]] * (host[5] > 0), minlength=S)
    args = (ipa, ixa, daa, T, H, ipn, ixn, dan)
    ptr, loc = cell_support(*args)
    n_slots = int(ptr[-1])
    print("%d cells, %d ECs, %d non-zeros of A, %d entries of N; expanded %d non-zeros, %d slots (x %d haplotypes)"
          % (S, E, len(host[1]), len(host[4]), int(x_cell.sum()), n_slots, H))
    # two cells against the checker: one step from theta_0, and the stop
    import cell_quant_checker as cq
    import quant_checker as qchk
    picks = [0, S - 1]
    keep = np.zeros(S, dtype=np.uint8)
    keep[picks] = 1
    one = quantify_cells(*args, cell_keep=keep, max_iters=1, tol=0.0)
    full = quantify_cells(*args, cell_keep=keep)
    for c in picks:
        cell = cq.Cell(host[0], host[1], host[2], T, H, host[3], host[4], host[5], c)
        ref, ex = cell.step(cell.p.aln())
        p1, th1 = np.asarray(one[0].cpu() if hasattr(one[0], "cpu") else one[0]), np.asarray(one[2].cpu() if hasattr(one[2], "cpu") else one[2])
        worst = qchk.agree(cell.scatter(th1[p1[c]:p1[c + 1]]), ref, cell.tolerance())
        _, ri = cell.run()
        print("cell %d: one step within %.3g of the checker's (bound %.3g), explained %d = %d; to tol 1e-6: %d steps (checker %d)"
              % (c, worst, cell.tolerance(), int(one[3]["explained"][c]), ex, int(full[3]["n_iter"][c]), ri["n_iter"]))
        assert abs(int(full[3]["n_iter"][c]) - ri["n_iter"]) <= 1
    print("wall time of the call with its waits, warm, ms:")
    print("  cell_support                          %s" % _fmt(wall(lambda: cell_support(*args))))
    t0 = wall(lambda: quantify_cells(*args, max_iters=0, n_slots=n_slots))
    print("  quantify_cells,  0 steps (the set-up) %s" % _fmt(t0))
    t8 = wall(lambda: quantify_cells(*args, max_iters=8, tol=0.0, n_slots=n_slots))
    print("  quantify_cells,  8 steps              %s" % _fmt(t8))
    t24 = wall(lambda: quantify_cells(*args, max_iters=24, tol=0.0, n_slots=n_slots))
    print("  quantify_cells, 24 steps              %s" % _fmt(t24))
    per_step = (np.median(t24) - np.median(t8)) / 16
    nbytes = step_bytes(int(x_cell.sum()), int((host[5] > 0).sum()), n_slots * H, n_slots)
    print("  per step, every cell running (24 against 8 steps, medians): %.1f us; algorithmic bytes %.2f GB = %.2f TB/s = %.0f %% of the %g TB/s HBM peak"
          % (per_step * 1e3, nbytes / 1e9, nbytes / (per_step * 1e-3) / 1e12, 100 * nbytes / (per_step * 1e-3) / HBM_PEAK, HBM_PEAK / 1e12))
    res = quantify_cells(*args, n_slots=n_slots)
    tf = wall(lambda: quantify_cells(*args, n_slots=n_slots))
    info = {k: np.asarray(v.cpu() if hasattr(v, "cpu") else v) for k, v in res[3].items()}
    n = info["n_iter"].astype(np.int64)
    launched = -(-int(n.max()) // 8) * 8
    print("  quantify_cells to tol 1e-6, all %d cells %s" % (S, _fmt(tf)))
    print("  steps per cell: min %d, median %d, max %d; %d of %d cells converged; steps launched %d" % (n.min(), np.median(n), n.max(), info["converged"].sum(), S, launched))
    useful = float((n * x_cell).sum())
    print("  share of the launched work (steps x expanded non-zeros) that fell on cells already done: %.1f %%"
          % (100 * (1 - useful / (launched * x_cell.sum()))))
    # the yardstick: the code as it was, one call per cell
    rng = np.random.default_rng(4)
    cells = np.sort(rng.choice(S, size=min(sample, S), replace=False))
    quantify(*args, sample=int(cells[0]))
    ts, its = [], []
    for c in cells:
        t = wall(lambda: its.append(quantify(*args, sample=int(c))[1]["n_iter"]), 1)
        ts += t
    total = float(np.sum(ts))
    print("yardstick, ecb.quantify(sample=c, tol=1e-6) on %d seeded cells: %.1f ms in all (per cell: median %.1f ms, %d steps); x %d / %d = %.0f ms for all cells"
          % (len(cells), total, np.median(ts), np.median(its), S, len(cells), total * S / len(cells)))
    print("quantify_cells for all %d cells: %.1f ms (cell_support %.1f ms before it when the caller does not know n_slots): %.1f times faster"
          % (S, np.median(tf), np.median(wall(lambda: cell_support(*args), 1)), total * S / len(cells) / np.median(tf)))
    dn = res[3]["n_iter"][[int(c) for c in cells]]
    dn = np.asarray(dn.cpu() if hasattr(dn, "cpu") else dn).astype(np.int64)
    print("steps of those cells, the batched call against the loop: largest difference %d" % int(np.abs(dn - np.array(its)).max()))


def gene_map(T, seed=4):
    """(gene[t], G): T / 4 genes, every target's drawn with a seed; ids renumbered so that none is empty."""
    rng = np.random.default_rng(seed)
    ids, gene = np.unique(rng.integers(0, max(T // 4, 1), size=T), return_inverse=True)
    return gene.astype(np.int32), len(ids)


def report_models(a, T, H, S, quantify_cells, quantify_cells_model, cell_support, wall):
    ipa, ixa, daa, ipn, ixn, dan = a
    host = [np.asarray(t.cpu() if hasattr(t, "cpu") else t) for t in a]
    args = (ipa, ixa, daa, T, H, ipn, ixn, dan)
    gene, G = gene_map(T)
    n_slots = int(cell_support(*args)[0][-1])
    members = np.bincount(gene, minlength=G)
    print("%d cells, %d entries of N, %d slots (x %d haplotypes); %d genes over %d targets, %d to %d members"
          % (S, len(host[4]), n_slots, H, G, T, members.min(), members.max()))
    import cell_model_checker as cm
    import cell_quant_checker as cq
    import quant_checker as qchk
    picks = [0, S - 1]
    keep = np.zeros(S, dtype=np.uint8)
    keep[picks] = 1
    qs = {c: cm.CellGrouping(cq.Cell(host[0], host[1], host[2], T, H, host[3], host[4], host[5], c), gene, G) for c in picks}
    np_ = lambda v: np.asarray(v.cpu() if hasattr(v, "cpu") else v)      # noqa: E731
    for model in (1, 2, 3):
        one = quantify_cells_model(*args, gene=gene, n_genes=G, model=model, cell_keep=keep, max_iters=1, tol=0.0)
        for c in picks:
            q = qs[c]
            ref, ex = q.step(model, q.p.aln())
            p1, th1 = np_(one[0]), np_(one[2])
            worst = qchk.agree(q.cell.scatter(th1[p1[c]:p1[c + 1]]), ref, q.tolerance(model))
            print("model %d, cell %d: one step within %.3g of the checker's (bound %.3g; M %d, R %d), explained %d = %d"
                  % (model, c, worst, q.tolerance(model), q.M, q.R, int(np_(one[3]["explained"])[c]), ex))
    print("wall time of the call with its waits, warm, ms (0 steps = the set-up; per step = (24 steps - 8 steps) / 16, medians, every cell running):")
    runs = [("flat (quantify_cells)", lambda **kw: quantify_cells(*args, n_slots=n_slots, **kw))]
    runs += [("model %d" % model, lambda model=model, **kw: quantify_cells_model(*args, gene=gene, n_genes=G, model=model, n_slots=n_slots, **kw)) for model in (1, 2, 3)]
    flat = None
    for name, call in runs:
        call(max_iters=8, tol=0.0)                                      # (warm: every kernel of this path loaded, the scratch grown)
        t0, t8, t24 = (wall(lambda: call(max_iters=k, tol=0.0)) for k in (0, 8, 24))
        per_step = (np.median(t24) - np.median(t8)) / 16
        flat = flat or (per_step, float(np.median(t0)))
        print("  %-22s  0 steps %s" % (name, _fmt(t0)))
        print("  %-22s  8 steps %s" % ("", _fmt(t8)))
        print("  %-22s 24 steps %s" % ("", _fmt(t24)))
        print("  %-22s per step %.2f ms = %.2f x the flat step; set-up %.1f ms = %.2f x the flat set-up"
              % ("", per_step, per_step / flat[0], np.median(t0), np.median(t0) / flat[1]))


def main():
    mode = sys.argv[1]
    import select_c4
    if mode == "rehearse":
        import cell_quant_checker as cq
        import quant_checker as qchk
        select_c4.E, select_c4.T, select_c4.H, select_c4.S = 3000, 400, 2, 12
        a = [t.numpy() for t in select_c4.inputs(device="cpu", sizes=(20, 61))]

        def fake_quantify(*args, sample=None, **kw):
            return qchk.run(qchk.Problem(*args, sample=sample), **kw)
        report(a, 400, 2, 12, 3000, lambda *x, n_slots=None, **kw: cq.quantify_cells(*x, **kw), lambda *x: cq.quantify_cells(*x, max_iters=0)[:2],
               fake_quantify, _cpu_wall, sample=4)
        import cell_model_checker as cm
        report_models(a, 400, 2, 12, lambda *x, n_slots=None, **kw: cq.quantify_cells(*x, **kw), lambda *x, n_slots=None, **kw: cm.quantify_cells_model(*x, **kw),
                      lambda *x: cq.quantify_cells(*x, max_iters=0)[:2], _cpu_wall)
        return
    import torch
    from alntools_amd import ecb
    S = int(sys.argv[2]) if len(sys.argv) > 2 else select_c4.S
    a = select_c4.inputs()
    if S < select_c4.S:
        n = int(a[3][S])
        a[3], a[4], a[5] = a[3][:S + 1].contiguous(), a[4][:n].contiguous(), a[5][:n].contiguous()
    print("box %s, %s" % (socket.gethostname(), torch.cuda.get_device_name(0)))
    if mode == "one":
        K = int(sys.argv[3]) if len(sys.argv) > 3 else 16
        if len(sys.argv) > 4:
            gene, G = gene_map(select_c4.T)
            r = ecb.quantify_cells_model(a[0], a[1], a[2], select_c4.T, select_c4.H, a[3], a[4], a[5], gene=gene, n_genes=G, model=int(sys.argv[4]),
                                         max_iters=K, tol=0.0)
        else:
            r = ecb.quantify_cells(a[0], a[1], a[2], select_c4.T, select_c4.H, a[3], a[4], a[5], max_iters=K, tol=0.0)
        torch.cuda.synchronize()
        print(int(r[0][-1]), "slots")
        return
    if mode == "models":
        report_models(a, select_c4.T, select_c4.H, S, ecb.quantify_cells, ecb.quantify_cells_model, ecb.cell_support, _wall)
        return
    report(a, select_c4.T, select_c4.H, S, select_c4.E, ecb.quantify_cells, ecb.cell_support, ecb.quantify, _wall)


if __name__ == "__main__":
    main()
