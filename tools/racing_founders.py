#!/usr/bin/env python
"""Which race outcomes the slices-aligned streams of tests/racing_streams.py reach: every family once through ks_std, ks_par and ks_short
with the -DECB_TIMING build, whose k_stream counts, per batch, the claims its flush lost to another hash and to the same hash, the lanes
that went through table_settle and those it sent on (ST_OTHER).  The library prints the counts on stderr ("[ecb timing] ... [race] ...");
this script catches them per run, checks the run against the C oracle and prints one line per family and compilation.  The same four for
the callers of table_lookup -- k_slow behind the push, and k_merge over the eight shards of racing_streams.merge_shard -- come from the
build's device-wide words (ecb_timing_race), which k_stream does not touch.

    tools/tools_variants.sh build "timing:-DECB_TIMING"
    ECB_LIB=libecb_timing.so python tools/racing_founders.py [family ...] > racing_founders.txt

profiles/racing_founders.txt is its output."""
import os
import re
import sys
import tempfile

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

RACE = re.compile(r"\[race\] claims lost to another hash (\d+), to the same hash (\d+); lanes in table_settle (\d+), of them ST_OTHER (\d+)")
KNOBS = {"ks_std": ("ECB_NO_PAR",), "ks_par": ("ECB_FORCE_PAR",), "ks_short": ("ECB_FORCE_SHORT",)}
# families that must show lost claims and settles at their committed shape; same_hash must show ST_OTHER too
MUST = ("same_order", "rotated", "same_slot", "same_hash", "long_keys")


def captured(fn):
    """fn() with the process's stderr (the library's fprintf) going to a file -> its text."""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        return f.read().decode(errors="replace")


def others(lib):
    """The race counters of k_slow and k_merge since the last call (which zeroes them)."""
    import ctypes as C
    out = (C.c_ulonglong * 4)()
    rc = lib.ecb_timing_race(0, out)
    assert rc == 0, rc
    return list(out)


def merges(ecb, rs, lib, torch):
    """Eight shards of the same reads into one root: whole in one k_merge launch, and by two key ranges."""
    from alntools_amd import dist as ecdist
    from oracle import c_oracle
    from test_gpu_flush_rounds import _check
    dev = torch.device("cuda:0")
    t, info = rs.merge_shard()
    w = rs.concatenated(t)
    exp = c_oracle.ec_from_tuples(w["read_id"], w["locus"], w["hapflag"], rs.H, threads=4)
    d = [torch.from_numpy(t[k].view(np.int32).copy()).cuda() for k in ("read_id", "locus", "hapflag")]
    whole, parts, totals, base = [], [], [0, 0, 0], 0
    for _ in range(rs.N_SHARDS):
        with ecb.EcBuilder(rs.T, rs.H) as b:
            b.push_device(*d)
            eng = ecdist.GpuEngine(b, dev)
            ne, npairs, nreads = b.table_sizes()
            whole.append(eng.table_export(base) + (ne, npairs))
            parts.append(eng.table_export_parts(base, 2))
            totals = [x + y for x, y in zip(totals, b.counters())]
            base += nreads
    others(lib)
    print("# k_merge: eight shards of the same %d keys (tests/racing_streams.py: merge_shard) into an empty root of the shards' capacity" % info["n_ecs"])
    print("%-28s %8s %10s %10s %8s %9s" % ("merge", "n_ecs", "lost_other", "lost_same", "settle", "st_other"))
    with ecb.EcBuilder(rs.T, rs.H) as root:
        ecdist.GpuEngine(root, dev).table_merge_many([(ent, ne, prs, npairs) for ent, prs, ne, npairs in whole])
        c = others(lib)
        root.add_counters(*totals)
        _check(root.export(), root.finalize(), exp)
    print("%-28s %8d %10d %10d %8d %9d" % ("whole, one launch", info["n_ecs"], c[0], c[1], c[2], c[3]))
    got = [c]
    for q in range(2):
        with ecb.EcBuilder(rs.T, rs.H) as part:
            ecdist.GpuEngine(part, dev).table_merge_many([(ent[eo[q] * 4:eo[q + 1] * 4], eo[q + 1] - eo[q], prs[po[q]:po[q + 1]], po[q + 1] - po[q])
                                                          for ent, prs, eo, po in parts])
            c = others(lib)
            n = part.table_sizes()[0]
        print("%-28s %8d %10d %10d %8d %9d" % ("key range %d of 2, one launch" % q, n, c[0], c[1], c[2], c[3]))
        got.append(c)
    return got


def main(names):
    if "timing" not in os.environ.get("ECB_LIB", ""):
        sys.exit("run with ECB_LIB=libecb_timing.so (tools/tools_variants.sh build \"timing:-DECB_TIMING\")")
    import torch
    from alntools_amd import ecb
    import racing_streams as rs
    from test_gpu_flush_rounds import _check
    print("# race outcomes of k_stream's flush per family and compilation, one device push each (tools/racing_founders.py, -DECB_TIMING build)")
    print("# lost_other: claims that found the slot taken by another hash | lost_same: by a founder with the same hash | settle: lanes through")
    print("# table_settle | st_other: settles that ended on the other key of the hash (counts over all launches of the push: growth parks and resumes)")
    print("%-18s %-9s %7s %8s %10s %10s %8s %9s" % ("family", "kernel", "slices", "n_ecs", "lost_other", "lost_same", "settle", "st_other"))
    short = []
    lib = ecb.load()
    slow = []
    for name in names:
        t, info, exp = rs.family(name)
        d = [torch.from_numpy(t[k].view(np.int32).copy()).cuda() for k in ("read_id", "locus", "hapflag") + (("pos",) if "pos" in t else ())]
        for kernel, env in KNOBS.items():
            if "pos" in t and kernel != "ks_std":
                continue                                   # (track_ranges has one compilation)
            for k in sum(KNOBS.values(), ()):
                os.environ.pop(k, None)
            for k in env:
                os.environ[k] = "1"
            kw = dict(ec_capacity=rs.CAP_SMALL) if name in rs.SMALL_TABLE else {}
            with ecb.EcBuilder(rs.T, rs.H, track_ranges="pos" in t, **kw) as b:
                if kernel == "ks_short":
                    b.hint_reads(t["n_reads"])
                others(lib)
                text = captured(lambda: b.push_device(*d))
                slow.append((name, kernel, others(lib)))
                ran = b.profile_kernel()
                _check(b.export(), b.finalize(), exp)
            rows = [tuple(int(x) for x in m) for m in RACE.findall(text)]
            assert rows and ran.startswith(kernel + "::"), (name, kernel, ran, text[-400:])
            c = [sum(r[i] for r in rows) for i in range(4)]
            print("%-18s %-9s %7d %8d %10d %10d %8d %9d" % (name, kernel, t["n_slices"], info["n_ecs"], c[0], c[1], c[2], c[3]))
            base = name.replace("_256", "")
            if base in MUST and (c[0] + c[1] == 0 or c[2] == 0 or (base == "same_slot" and c[0] == 0) or (base == "same_hash" and (c[1] == 0 or c[3] == 0))):
                short.append((name, kernel))
    print("# k_slow behind the same pushes (the reads k_stream deferred: the giants, and in growth the reads that met a full table); settle = lookups")
    print("# that met their hash in a slot and compared keys (same_key), st_other = those that found the other key")
    print("%-18s %-9s %10s %10s %8s %9s" % ("family", "kernel", "lost_other", "lost_same", "settle", "st_other"))
    for name, kernel, c in slow:
        if any(c):
            print("%-18s %-9s %10d %10d %8d %9d" % (name, kernel, c[0], c[1], c[2], c[3]))
    print("# (every other push: 0 0 0 0 -- it deferred no read)")
    if len(names) == len(rs.FAMILIES):
        merges(ecb, rs, lib, torch)
    print("# condition (lost claims > 0 and settles > 0 for %s; to another hash for same_slot; to the same hash and ST_OTHER > 0 for same_hash): %s"
          % (", ".join(MUST), "met" if not short else "NOT met by %s" % short))
    return 1 if short else 0


if __name__ == "__main__":
    import racing_streams
    sys.exit(main(sys.argv[1:] or sorted(racing_streams.FAMILIES)))
