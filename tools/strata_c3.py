# -*- coding: utf-8 -*-
"""Input and timing of profiles/best_strata_c3.txt: config 3's record stream from ``alntools_amd/synth.py`` (100 M paired-end reads,
80 000 transcripts x 8 haplotypes) with a seeded score in 0 .. 3 per record, through ``ecb_best_strata_device``.

    python tools/strata_c3.py [N_READS]            (default 100 000 000)
    python tools/strata_c3.py N_READS once         the warm-up call and one more, for a kernel trace of its own

Reports, from one process: the HIP-event time of the whole warm device call, out of place, "lowest" -- kernels, the library's two
read-backs and waits -- five calls after the one that grows the pool; the same in place; device-to-device copies as the floor (a
buffer of 20 bytes per record -- 20 read and 20 written --, and one of 10 bytes per record, which moves the 20 bytes per record that
the call moves at the least: 12 in, 8 out); and the call on a leading slice next to ``tests/strata_checker.py``, the results compared.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
CHUNK_READS = 1 << 20
SLICE = 200_000


def stream(n_reads, device):
    """read_id, hapflag and score of config 3's first ``n_reads`` reads as int32 CUDA tensors in ONE allocation."""
    import torch
    from alntools_amd import synth
    spec = synth.SynthSpec(n_reads, 80_000, 8, paired=True)
    n = synth.count_records(spec, 0, n_reads, device=device)
    stride = (n + 3) // 4 * 4
    arena = torch.empty(3 * stride, dtype=torch.int32, device=device)
    rid, hf, sc = arena[:n], arena[stride:stride + n], arena[2 * stride:2 * stride + n]
    at, reads = 0, 0
    for a in range(0, n_reads, CHUNK_READS):
        g = synth.generate(spec, a, min(a + CHUNK_READS, n_reads), device=device, read_id_base=reads)
        m = g["n_records"]
        rid[at:at + m] = g["read_id"]
        hf[at:at + m] = g["hapflag"]
        idx = torch.arange(at, at + m, dtype=torch.int64, device=device)
        sc[at:at + m] = (((idx * 2654435761 + 20260101) >> 13) & 3).to(torch.int32)       # seeded: a hash of the record's index
        at += m
        reads += g["n_reads"]
        del g, idx
    assert at == n
    return rid, hf, sc, reads


def main(n_reads, once=False):
    import torch
    import bus_c4
    import strata_checker as sk
    from alntools_amd import ecb_strata as es
    fmt = lambda ts: " / ".join("%.3f" % t for t in ts)   # noqa: E731
    t0 = time.perf_counter()
    rid, hf, sc, reads = stream(n_reads, torch.device("cuda", 0))
    torch.cuda.synchronize()
    n = rid.numel()
    print("records: %d of %d reads (%.2f GB in the three streams), made in %.1f s" % (n, reads, 12 * n / 1e9, time.perf_counter() - t0), flush=True)
    out_rid, out_hf, counts = es.best_strata(rid, hf, sc, lowest=True)                   # (warm-up: the pool grows here)
    print("counts (passing, kept, dropped, reads whose first passing record was dropped): %r" % (counts,), flush=True)
    if once:
        es.best_strata(rid, hf, sc, lowest=True)
        torch.cuda.synchronize()
        return
    gbs = lambda ms, bytes_per_record: bytes_per_record * n / ms / 1e6   # noqa: E731
    wall, ev = bus_c4._timed(lambda: es.best_strata(rid, hf, sc, lowest=True))
    best = min(ev)
    print("ecb_best_strata_device, out of place  wall ms: %s   HIP events ms: %s   (min %.3f ms: %.1f ps per record; %.0f GB/s of the 20 bytes per "
          "record it must move, %.0f GB/s of the 32 it does move)" % (fmt(wall), fmt(ev), best, best * 1e9 / n, gbs(best, 20), gbs(best, 32)), flush=True)
    del out_rid, out_hf
    for name, per in (("20 bytes per record (20 read, 20 written)", 20), ("10 bytes per record (10 read, 10 written: the 20 the call must move)", 10)):
        src = torch.empty(per * n // 4 + 1, dtype=torch.int32, device="cuda").fill_(7)
        dst = torch.empty_like(src)
        _, cev = bus_c4._timed(lambda: dst.copy_(src))
        print("device-to-device copy of %s  HIP events ms: %s   (min %.3f ms: %.0f GB/s moved)   the call is %.2f times that"
              % (name, fmt(cev), min(cev), gbs(min(cev), 2 * per), best / min(cev)), flush=True)
        del src, dst
    # the leading slice against the checker (cut at a read boundary), then in place -- which spends the input
    k = es.cut_whole_reads(rid[:SLICE].cpu().numpy().view(np.uint32))
    part = [t[:k].cpu().numpy() for t in (rid, hf, sc)]
    got = es.best_strata(rid[:k].clone(), hf[:k].clone(), sc[:k].clone(), lowest=True)
    want = sk.best_strata(part[0].view(np.uint32), part[1].view(np.uint32), part[2], lowest=True)
    print("the first %d records against tests/strata_checker.py: equal: %s" % (k, np.array_equal(got[0].cpu().numpy().view(np.uint32), want[0]) and
                                                                            np.array_equal(got[1].cpu().numpy().view(np.uint32), want[1]) and got[2] == want[2]), flush=True)
    keep_rid, keep_hf = rid.clone(), hf.clone()

    def in_place():
        rid.copy_(keep_rid)
        hf.copy_(keep_hf)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        es.best_strata(rid, hf, sc, lowest=True, inplace=True)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)
    iev = [in_place() for _ in range(5)]
    print("ecb_best_strata_device, in place  HIP events ms: %s   (min %.3f ms)" % (fmt(iev), min(iev)), flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000, once=len(sys.argv) > 2 and sys.argv[2] == "once")
