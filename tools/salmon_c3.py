# -*- coding: utf-8 -*-
"""Input and timing of profiles/salmon2ec_c3.txt: a config-3-sized salmon directory (80 000 transcripts x 8 haplotypes = 640 000 targets
in shuffled header order, 3.7 M ECs, ~40 M target ids; tests/salmon_checker.py's writer, seed 33) -- ``python tools/salmon_c3.py write
DIR [N_ECS]`` -- and the command's wall time split into file read, header + quant.sf parse, ecb.salmon_ecs (cold, then warm) and .bin
write -- ``python tools/salmon_c3.py time DIR``."""
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def write(d, n_ecs=3_700_000):
    import salmon_checker as chk
    rng = np.random.default_rng(33)
    names = chk.target_names(80_000, list("ABCDEFGH"), rng)
    eff = rng.uniform(0, 5000, size=len(names))
    ptr, tid, counts = chk.random_ecs_fast(rng, len(names), int(n_ecs))
    section = chk.ec_section(ptr, tid, counts)
    chk.write_salmon_dir(d, names, eff, section, int(n_ecs))
    print("%s: %d targets, %d ECs, %d target ids, %.1f MB of EC lines" % (d, len(names), n_ecs, len(tid), len(section) / 1e6))


def timed(d):
    os.environ.setdefault("ALNTOOLS_TORCH", "0")
    from alntools_amd import bin_utils, ecb, salmon_utils
    t0 = time.perf_counter()
    path = salmon_utils.eq_classes_path(d)
    data = salmon_utils.read_eq_classes(path)
    t1 = time.perf_counter()
    hdr = salmon_utils.parse_header(data, path)
    lname, hname, col, hap = salmon_utils.number_targets(hdr.names, (), path)
    eff = salmon_utils.read_lengths(os.path.join(d, "quant.sf"), hdr.names)
    lengths = np.zeros((len(lname), len(hname)), dtype=np.int64)
    lengths[col, hap] = eff
    section = np.frombuffer(data, dtype=np.uint8, offset=hdr.ec_offset)
    ecb.load()
    t2 = time.perf_counter()
    out = ecb.salmon_ecs(section, hdr.n_ecs, col, hap, len(lname), len(hname))
    t3 = time.perf_counter()
    reps = []
    for _ in range(3):
        a = time.perf_counter()
        ecb.salmon_ecs(section, hdr.n_ecs, col, hap, len(lname), len(hname))
        reps.append(time.perf_counter() - a)
    t4 = time.perf_counter()
    ip, ix, da, nix, nda = out
    m = bin_utils.ECMatrices(hname, lname, lengths, ["NA"], ip, ix, da, np.array([0, len(nix)], np.int32), nix, nda)
    with open(os.path.join(d, "timed_out.bin"), "wb") as f:
        f.write(bin_utils.ecsave2_bytes(m))
    t5 = time.perf_counter()
    print("bytes %d  ECs %d  targets %d  -> nnz A %d  nnz N %d" % (len(data), hdr.n_ecs, hdr.n_targets, len(ix), len(nix)))
    print("file read %.3f s, header + names + quant.sf + library load %.3f s, salmon_ecs cold (host arrays, copies included) %.3f s, "
          "warm %s s, encode + write %.3f s" % (t1 - t0, t2 - t1, t3 - t2, " / ".join("%.3f" % r for r in reps), t5 - t4))


if __name__ == "__main__":
    if sys.argv[1] == "write":
        write(sys.argv[2], *(int(a) for a in sys.argv[3:4]))
    else:
        timed(sys.argv[2])
