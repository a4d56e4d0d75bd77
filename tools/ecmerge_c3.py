# -*- coding: utf-8 -*-
"""Inputs and timing of profiles/ecmerge_c3.txt: four config-3-sized .bin files (tests/gt_checker.py:c3_csr, 3.7 M rows and 13 M
non-zeros each, seeds 3 .. 6, one sample each under its own name) -- ``python tools/ecmerge_c3.py write DIR`` -- and the command's wall
time split into load, device and write -- ``python tools/ecmerge_c3.py time DIR``."""
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def write(d):
    import gt_checker
    from alntools_amd import bin_utils
    os.makedirs(d, exist_ok=True)
    paths = []
    for k, seed in enumerate((3, 4, 5, 6)):
        ip, ix, da, T, H = gt_checker.c3_csr(seed)
        E = len(ip) - 1
        rng = np.random.default_rng(seed)
        count = rng.integers(0, 100, size=E).astype(np.int32)
        nz = np.flatnonzero(count).astype(np.int32)
        lname = ["ENSMUST%011d" % t for t in range(T)]
        lengths = np.random.default_rng(0).integers(200, 5000, size=(T, H))
        m = bin_utils.ECMatrices(list("ABCDEFGH")[:H], lname, lengths, ["c3_%d" % k], ip, ix, da, np.array([0, len(nz)], np.int32), nz, count[nz])
        p = os.path.join(d, "c3_%d.bin" % k)
        bin_utils.ecsave2(p, m)
        paths.append(p)
    print("\n".join(paths))


def timed(d):
    os.environ.setdefault("ALNTOOLS_TORCH", "0")
    from alntools_amd import bin_utils, ecb
    files = sorted(os.path.join(d, f) for f in os.listdir(d) if f.startswith("c3_") and f.endswith(".bin"))
    t0 = time.perf_counter()
    ms = [bin_utils.ecload(f) for f in files]
    plan = bin_utils.plan_merge(ms, files)
    t1 = time.perf_counter()
    parts = [dict(indptrA=m.indptrA, indicesA=m.indicesA, dataA=m.dataA, indptrN=m.indptrN, indicesN=m.indicesN, dataN=m.dataN,
                  n_loci=m.num_loci, target_map=tm, sample_map=sm) for m, tm, sm in zip(ms, plan.target_maps, plan.sample_maps)]
    ecb.load()
    t2 = time.perf_counter()
    out = ecb.combine(parts, len(plan.lname), len(plan.hname), len(plan.sname))
    t3 = time.perf_counter()
    reps = []
    for _ in range(3):
        a = time.perf_counter()
        ecb.combine(parts, len(plan.lname), len(plan.hname), len(plan.sname))
        reps.append(time.perf_counter() - a)
    b = bin_utils.ecsave2_bytes(bin_utils.ECMatrices(plan.hname, plan.lname, plan.lengths, plan.sname, *out))
    with open(os.path.join(d, "timed_out.bin"), "wb") as f:
        f.write(b)
    t4 = time.perf_counter()
    print("rows %d  pairs %d  -> ECs %d  nnz A %d  nnz N %d" % (sum(m.num_reads for m in ms), sum(len(m.indicesA) for m in ms),
                                                          len(out[0]) - 1, len(out[1]), len(out[4])))
    print("load + plan %.3f s, library load %.3f s, first combine (host arrays, copies included) %.3f s, warm %s s, encode + write %.3f s"
          % (t1 - t0, t2 - t1, t3 - t2, " / ".join("%.3f" % r for r in reps), t4 - t3 - sum(reps)))


if __name__ == "__main__":
    {"write": write, "time": timed}[sys.argv[1]](sys.argv[2])
