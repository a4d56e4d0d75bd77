# -*- coding: utf-8 -*-
"""Drop-in for the reference's ``alntools/bam_utils_multisample.py``: a directory of BAM files, one EC x cell
count matrix (``convert`` keeps the signature of ``bam_utils_multisample.py:357``).

Split of the work:
* host -- what needs names: header maps, read runs and the cell of every read (field 14 of the ``'|||'``-separated
  read name, ``:270-280``), per file, with the reference's quirks kept: after the first read of a file the tracked
  name is the UNTRIMMED query name (``:292``), and the last read of every file is never counted (``:306-321``);
* device (libecb) -- everything read-sized: filter, target sets, ECs in first-appearance order, A, and the reduction
  of reads to distinct (EC, cell, file) triples with counts and first read index (``ec[key][cell] += 1``, ``:288-290``);
* device too (``ecb_ms_filter``): cell order (``cr_totals`` insertion order, ``:513-546``), the minimum-count filter and EC
  re-ranking (``:596-636``), N as CSC (``:737-791``), from the triples; the host only maps cell ids back to names.

File order: the reference takes ``glob.glob`` order (``:379``), which is filesystem-dependent and changes sample
order and EC order; ``convert`` here sorts the file names.  ``convert_files`` takes an explicit order.
"""
from __future__ import annotations

import glob
import os
import time

import numpy as np

from . import utils
from .bam_utils import BATCH_RECORDS, ec_matrices, header_maps, open_bam, replace_bin, write_range_file
from .ecb import FLAG_MATE_OTHER_REF, FLAG_NEXT_POS_NEG, HAP_SHIFT, EcBuilder, EcbError
from .tuples import record_valid, trim_name

LOG = utils.get_logger()
CELL_BITS = 22


class CollapseUmisError(ValueError):
    """What ``--collapse-umis`` refuses: a combination it does not run with, a run beyond the record limit."""


def umi_refusal(multisample=True, range_filename=None):
    """Why ``--collapse-umis`` does not run as asked, in words that name the option -- or None."""
    if not multisample:
        return "--collapse-umis needs --multisample: the cell and the UMI are fields of the multisample read names"
    if range_filename:
        return "--collapse-umis does not run with --rangefile: the ranges are defined over alignments that the collapse removes"
    if int(os.environ.get("ALNTOOLS_GPUS", "1") or 1) > 1:
        return "--collapse-umis does not run with ALNTOOLS_GPUS above 1"
    return None


def scan_file(reader, maps, scored=False, umis=False):
    """One BAM file -> (tuples of its counted reads, cell name per counted read, counters, dropped-run records).

    Restates the name logic of ``bam_utils_multisample.py:257-300`` on the valid records of the file.  ``scored``: the reader works
    out every record's score (``set_score``); the columns then hold ``score`` and ``present`` too.  ``umis``: a fifth value follows,
    the raw UMI of every counted read next to its cell -- field 6 of the same tracked name, as it stands (``--collapse-umis``).
    """
    run_umis = []
    done = (lambda *r: r + (run_umis[:max(run, 0)],)) if umis else (lambda *r: r)
    if umis and hasattr(reader, "read_ms"):
        reader.set_umi(True)
    cols = {k: [] for k in ("flag", "tid", "pos", "ntid", "npos", "run") + (("score", "present") if scored else ())}
    run_cells = []
    tracked, run = None, -1
    n_all = n_valid = 0
    while hasattr(reader, "read_ms"):                                  # native decoder: the same rule, applied where the names are
        d, cells = reader.read_ms(BATCH_RECORDS)
        if d is None:
            c = {k: (np.concatenate(v) if v else np.zeros(0, dtype=np.int64)) for k, v in cols.items()}
            return done(c, c["run"] < run, run_cells[:max(run, 0)], dict(all=n_all, valid=n_valid))
        runs = run + np.cumsum(d["newrun"], dtype=np.int64)
        run = int(runs[-1])
        run_cells.extend(cells)
        if umis:
            run_umis.extend(reader.ms_umis())
        n_all += len(runs)
        n_valid += int(d["valid"].sum())
        for k, v in (("flag", d["flag"]), ("tid", d["tid"]), ("pos", d["pos"]), ("ntid", d["next_tid"]), ("npos", d["next_pos"]), ("run", runs)):
            cols[k].append(np.array(v))
        if scored:
            for k, v in zip(("score", "present"), reader.scores()):
                cols[k].append(v)
    while True:
        q, flag, tid, pos, ntid, npos = reader.read_batch(BATCH_RECORDS)
        if not q:
            break
        valid = record_valid(flag, tid.astype(np.int64), ntid.astype(np.int64), npos.astype(np.int64))
        runs = np.empty(len(q), dtype=np.int64)
        for i in range(len(q)):
            if valid[i]:
                name = q[i]
                if tracked is None:
                    tracked = trim_name(name)                         # :257-262
                    run, new = 0, True
                else:
                    new = False
                if tracked != trim_name(name):                        # :288
                    tracked = name                                    # untrimmed, :292
                    run += 1
                    new = True
                if new:
                    fields = tracked.split('|||')
                    if len(fields) < 15:
                        raise ValueError("read name %r has no cell id in '|||' field 14 (bam_utils_multisample.py:270-280)" % tracked)
                    run_cells.append(fields[14])
                    if umis:
                        run_umis.append(fields[6])
            runs[i] = run
        n_all += len(q)
        n_valid += int(valid.sum())
        for k, v in (("flag", flag), ("tid", tid), ("pos", pos), ("ntid", ntid), ("npos", npos), ("run", runs)):
            cols[k].append(v)
        if scored:
            for k, v in zip(("score", "present"), reader.scores()):
                cols[k].append(v)
    c = {k: (np.concatenate(v) if v else np.zeros(0, dtype=np.int64)) for k, v in cols.items()}
    keep = c["run"] < run                                             # the file's last read is never counted (:306-321)
    return done(c, keep, run_cells[:max(run, 0)], dict(all=n_all, valid=n_valid))


def _tuples(c, sel, maps, read_base):
    tid = c["tid"][sel].astype(np.int64)
    flag = c["flag"][sel].astype(np.int64)
    ntid, npos = c["ntid"][sel].astype(np.int64), c["npos"][sel].astype(np.int64)
    valid = record_valid(flag, tid, ntid, npos)
    safe = np.where(valid, tid, 0)
    hostbits = np.where(tid != ntid, FLAG_MATE_OTHER_REF, 0) | np.where(npos < 0, FLAG_NEXT_POS_NEG, 0)
    hapflag = (flag & 0xFFF) | hostbits | (maps.tid2hap[safe].astype(np.int64) << HAP_SHIFT)
    rid = c["run"][sel] + read_base                                   # -1 (before the first read) wraps to 0xFFFFFFFF only at base 0
    rid = np.where(c["run"][sel] < 0, read_base - 1, rid)
    return ((rid & 0xFFFFFFFF).astype(np.uint32), maps.tid2locus[safe].astype(np.uint32), hapflag.astype(np.uint32),
            c["pos"][sel].astype(np.int32), valid)


class _Gather(object):
    """The builder as :func:`_push_files` sees it under ``--collapse-umis``: what would be pushed is held -- the records, and every
    counted read's cell, file and UMI -- until the whole run is in, since a molecule's reads may lie in different files.
    :meth:`collapse_into` then makes the reads of one molecule one read on the GPU (``ecb_collapse_umis``) and pushes the result, the
    cells taken from every molecule's first read."""

    def __init__(self):
        self.streams, self.meta, self.umis, self.n_records, self.counts = [], [], [], 0, None

    def push(self, rid, loc, hf, pos=None):
        from .ecb_umi import MAX_RECORDS
        self.n_records += len(rid)
        if self.n_records > MAX_RECORDS:
            raise CollapseUmisError("--collapse-umis: more than {:,} records in the run (2^30 - 1: one call collapses them all)".format(MAX_RECORDS))
        self.streams.append((rid, loc, hf))

    def push_cells(self, meta, first_read, umis=()):
        self.meta.append(meta)
        self.umis.extend(umis)

    def collapse_into(self, b, maps, device):
        from . import ecb_umi
        if not self.n_records:
            return
        rid, loc, hf = (np.concatenate([s[k] for s in self.streams]) for k in range(3))
        meta = np.concatenate(self.meta) if self.meta else np.zeros(0, np.uint32)
        keys = ecb_umi.mol_keys(meta & np.uint32((1 << CELL_BITS) - 1), self.umis)
        rid, loc, hf, first, self.counts = ecb_umi.collapse_umis(rid, loc, hf, keys, maps.n_loci, maps.n_haplotypes, device=device)
        if len(rid):
            b.push(rid, loc, hf, None)
            b.push_cells(meta[first], 0)

    def log(self):
        from .ecb_umi import COUNT_NAMES
        if self.counts is not None:
            LOG.info("--collapse-umis: " + ", ".join("{:,} {}".format(v, k) for k, v in zip(COUNT_NAMES, self.counts)))


def _push_files(b, maps, files, track, cell_of, strata=None, umis=False):
    """Scan ``files`` = [(global file index, path), ...] in order and push their counted reads into ``b`` (read ids local to this
    handle, from 0).  ``cell_of(name) -> id`` hands out cell ids.  -> (n_all, n_valid, reads pushed, host-side range extremes of
    the reads the reference never counts -- the last read of every file, ``:306-321`` -- which its ranges still see, ``:249-253``).
    ``strata`` (a :class:`bam_utils.BestStrata`): the rule runs over every file's records, which are held whole, before they are split
    into counted reads and the last one -- that read, which only the ranges see, by the same rule; ``n_valid`` then counts what is kept.
    ``umis``: ``push_cells`` is handed every counted read's raw UMI as well (``b`` is then a :class:`_Gather`)."""
    n_all = n_valid = 0
    host_min = np.full((maps.n_loci, maps.n_haplotypes), np.iinfo(np.int32).max, dtype=np.int64)
    host_max = np.full((maps.n_loci, maps.n_haplotypes), np.iinfo(np.int32).min, dtype=np.int64)
    read_base = 0
    for fi, path in files:
        rd = open_bam(path, names=False, ms=True)
        if strata is not None:
            strata.attach(rd, path)
        scanned = scan_file(rd, maps, scored=strata is not None, umis=umis)
        c, keep, cells, ctr = scanned[:4]
        rd.close()
        n_all += ctr["all"]
        if strata is not None:
            _push_file_strata(b, maps, c, keep, track, read_base, strata, host_min, host_max)
            n_valid = strata.counts[1]
        else:
            n_valid += ctr["valid"]
            rid, loc, hf, pos, _ = _tuples(c, keep, maps, read_base)
            if len(rid):
                b.push(rid, loc, hf, pos if track else None)
        if strata is None and track and (~keep).any():            # ranges see every valid alignment, counted or not (:249-253)
            _, l2, h2, p2, v2 = _tuples(c, ~keep, maps, 0)
            hap = (h2.astype(np.int64) >> HAP_SHIFT) & 0xFF
            np.minimum.at(host_min, (l2[v2].astype(np.int64), hap[v2]), p2[v2])
            np.maximum.at(host_max, (l2[v2].astype(np.int64), hap[v2]), p2[v2])
        if cells:
            ids = np.asarray([cell_of(name) for name in cells], dtype=np.uint32)
            b.push_cells(ids | np.uint32(fi << CELL_BITS), read_base, *scanned[4:])              # (with ``umis``: the reads' UMIs go with their cells)
        read_base += len(cells)
    return n_all, n_valid, read_base, host_min, host_max


def _push_file_strata(b, maps, c, keep, track, read_base, strata, host_min, host_max):
    """One file's records with ``--best-strata``: the rule over all of them (the file is whole reads), then the counted reads pushed
    and the last read's kept alignments shown to the host-side ranges."""
    from .bam_utils import BestStrataError, strata_passes
    every = np.ones(len(keep), dtype=bool)
    rid, loc, hf, pos, valid = _tuples(c, every, maps, read_base)
    if not len(rid):
        return
    missing = np.flatnonzero(valid & (c["present"] == 0))
    if len(missing):
        raise BestStrataError("{} record {}: no {} tag".format(strata.filename, int(missing[0]), strata.tag_a))
    rid, hf = strata.apply(rid, hf, c["score"].astype(np.int32))
    if keep.any():
        b.push(rid[keep], loc[keep], hf[keep], pos[keep] if track else None)
    if track and (~keep).any():
        v2 = ~keep & strata_passes(hf)
        hap = (hf.astype(np.int64) >> HAP_SHIFT) & 0xFF
        np.minimum.at(host_min, (loc[v2].astype(np.int64), hap[v2]), pos[v2])
        np.maximum.at(host_max, (loc[v2].astype(np.int64), hap[v2]), pos[v2])


def _finish(maps, names, sizes, f, range_len, ec_filename, emase_filename, range_filename, device, n_all, n_valid, start_time):
    """The host's part after ``ecb_ms_filter``: names for the kept cells, the files."""
    if range_filename:
        write_range_file(range_filename, maps, range_len)
    kept = [int(c) for c in f["kept_cells"]]
    n_ecs_kept = len(f["indptrA"]) - 1
    LOG.info("Number of ECs after filtering : {:,}".format(n_ecs_kept))
    LOG.info("Number of cells after filtering: {:,}".format(len(kept)))
    m = ec_matrices(maps, [names[c] for c in kept], f)
    if emase_filename:                                                # (unlike the single-sample run: nothing said, an existing file left to the writer)
        from . import emase_h5
        emase_h5.save(emase_filename, m, title='Multisample APM', incidence_only=False, count_2d=True, device=device)   # :806; N is a csc matrix whatever S is (:783-791)
    if ec_filename:
        replace_bin(ec_filename, m)
    LOG.info("Done, total time: {}".format(utils.format_time(start_time, time.time())))
    return dict(all_alignments=n_all, valid_alignments=n_valid, n_ecs=n_ecs_kept, n_cells=len(kept),
                n_ecs_before=sizes["n_ecs"], n_cells_before=len(names), samples=[names[c] for c in kept])


def _log_counts(maps, n_valid, sizes, n_cells):
    LOG.info("Number of alignments: {:,}".format(n_valid))
    LOG.info("Number of main targets: {:,}".format(maps.n_loci))
    LOG.info("Number of haplotypes: {:,}".format(maps.n_haplotypes))
    LOG.info("Number of ECs: {:,}".format(sizes["n_ecs"]))
    LOG.info("Number of cells: {:,}".format(n_cells))


def _filter(b, n_cells, minimum_count):
    try:
        return b.ms_filter(n_cells, minimum_count)                    # cell order, filter, re-rank, N: on the device
    except EcbError as e:
        if e.code == -7:                                              # ECB_ERR_EMPTY
            raise ValueError("no cell reaches the minimum count")
        raise


def _header_maps(bam_files, target_filename):
    LOG.info("Parsing the header of {}...".format(bam_files[0]))
    rd = open_bam(bam_files[0])
    maps = header_maps(rd, target_filename)                           # header of the first file only (:399-465)
    rd.close()
    return maps


def convert_files(bam_files, ec_filename, emase_filename, minimum_count=-1, range_filename=None, target_filename=None, best_strata=None,
                  collapse_umis=False):
    """``bam_files`` in the given order -> ``.bin`` / ``.h5``; returns counters.  ``ALNTOOLS_GPUS=N``: the files are dealt out to
    N processes, one per GPU (the reference: one worker per file, ``bam_utils_multisample.py:473-480``).  ``collapse_umis``: the
    counted reads of all files -- after the last read of every file has been set aside, and after ``best_strata`` -- are gathered in
    file order and collapsed in one call (:class:`_Gather`); the minimum count then counts molecules."""
    start_time = time.time()
    if collapse_umis:                                                 # (refused here, by name, before anything starts)
        why = umi_refusal(True, range_filename)
        if why:
            raise CollapseUmisError(why)
    if not bam_files:
        raise ValueError("no bam files")
    if len(bam_files) > (1 << (32 - CELL_BITS)):
        raise ValueError("more than %d input files" % (1 << (32 - CELL_BITS)))
    strata = None
    if best_strata is not None:                                       # (refused here -- an unknown tag, ALNTOOLS_GPUS above 1 -- before anything starts)
        from .bam_utils import BestStrata
        strata = BestStrata(best_strata, int(os.environ.get("ALNTOOLS_GPU", "0")))
    n_gpus = int(os.environ.get("ALNTOOLS_GPUS", "1"))
    if n_gpus > 1:
        from .dist import spawn_ranks
        return spawn_ranks(n_gpus, _rank_convert, (list(bam_files), ec_filename, emase_filename, minimum_count, range_filename, target_filename))
    maps = _header_maps(bam_files, target_filename)
    cell_ids = {}

    def cell_of(name):
        if name not in cell_ids:
            if len(cell_ids) >= (1 << CELL_BITS):
                raise ValueError("more than %d distinct cells" % (1 << CELL_BITS))
            cell_ids[name] = len(cell_ids)
        return cell_ids[name]

    device = int(os.environ.get("ALNTOOLS_GPU", "0"))
    track = range_filename is not None
    with EcBuilder(maps.n_loci, maps.n_haplotypes, device=device, track_ranges=track, multisample=True) as b:
        gather = _Gather() if collapse_umis else None
        n_all, n_valid, _, host_min, host_max = _push_files(b if gather is None else gather, maps, list(enumerate(bam_files)), track, cell_of, strata, umis=collapse_umis)
        if gather is not None:
            gather.collapse_into(b, maps, device)
        sizes = b.finalize()
        names = list(cell_ids.keys())
        _log_counts(maps, n_valid, sizes, len(names))
        if strata is not None:
            strata.log()
        if gather is not None:
            gather.log()
        f = _filter(b, len(names), minimum_count)
        range_len = None
        if track:
            mn, mx = b.export_range_minmax()
            mn, mx = np.minimum(mn.astype(np.int64), host_min), np.maximum(mx.astype(np.int64), host_max)
            range_len = np.where(mx >= mn, mx - mn + 1, 0)
    return _finish(maps, names, sizes, f, range_len, ec_filename, emase_filename, range_filename, device, n_all, n_valid, start_time)


def _rank_convert(rank, job, bam_files, ec_filename, emase_filename, minimum_count, range_filename, target_filename):
    """One process per GPU.  Rank r takes the files ``[r F / world, (r + 1) F / world)`` -- contiguous, so the run's read order is
    the reference's file order -- and builds the EC table of their reads on its GPU; cell ids are agreed on first (names in the
    order the files bring them up: rank 0's cells first, then what rank 1 adds ...: the single process's ids); the tables are
    merged by key range over the process group (``dist.exchange_and_merge``), every rank finalizes the range it merged and rank 0
    places the rows, every rank reduces its reads to (EC, cell, file) triples against the merged ECs
    (``dist.exchange_multisample``), and rank 0 filters and writes."""
    import pickle
    import torch
    import torch.distributed as tdist
    from . import dist as ecdist
    start_time = time.time()
    with ecdist.Rank(rank, job) as rk:                                # (its patience: ranks scan files of very different sizes)
        world = rk.world
        maps = _header_maps(bam_files, target_filename)
        F = len(bam_files)
        mine = [(fi, bam_files[fi]) for fi in range(rank * F // world, (rank + 1) * F // world)]
        track = range_filename is not None
        local_names = {}

        def cell_of(name):                                            # (local ids for now: this rank's order of first appearance)
            if name not in local_names:
                local_names[name] = len(local_names)
            return local_names[name]

        # Cell ids must be the run's before the reads' cells go to the device: scan first for names only?  No -- the cells of a read
        # are pushed with local ids and translated on the device side of the wire: push_cells takes ids, so the files are scanned
        # into host arrays of local ids per file, the name lists are exchanged, and the ids are mapped before push_cells.
        b = EcBuilder(maps.n_loci, maps.n_haplotypes, device=rk.dev_index, track_ranges=track, multisample=True)
        pending = []                                                  # (first read, local cell ids | file << CELL_BITS) per file

        class _Deferred(object):                                      # the builder as _push_files sees it: cells wait for their ids
            def push(self, *a):
                b.push(*a)

            def push_cells(self, meta, first_read):
                pending.append((first_read, meta))

        n_all, n_valid, n_reads, host_min, host_max = _push_files(_Deferred(), maps, mine, track, cell_of)
        # the run's cell ids: names in rank order, each rank's in its own order of first appearance
        cell_ids = {}
        for blob in ecdist.all_gather_bytes(pickle.dumps(list(local_names.keys())), rk.wire):
            for name in pickle.loads(blob):
                if name not in cell_ids:
                    cell_ids[name] = len(cell_ids)
        if len(cell_ids) > (1 << CELL_BITS):
            raise ValueError("more than %d distinct cells" % (1 << CELL_BITS))
        names = list(cell_ids.keys())
        remap = np.asarray([cell_ids[n] for n in local_names.keys()], dtype=np.uint32) if local_names else np.zeros(0, np.uint32)
        for first_read, meta in pending:
            b.push_cells(remap[meta & np.uint32((1 << CELL_BITS) - 1)] | (meta & ~np.uint32((1 << CELL_BITS) - 1)), first_read)
        eng = rk.engine(b)
        # Every rank ranks and emits the key range it merged; the root only places the rows (``ecb_assemble_ranges_device``) and takes the
        # ECs' hashes off the finished rows for the second exchange -- it no longer adopts every merged table and finalizes alone.
        # (ALNTOOLS_DIST_FINALIZE=root: the earlier ending, the merged tables adopted by the root.)
        per_range = os.environ.get("ALNTOOLS_DIST_FINALIZE", "ranges") != "root"
        merged = ecdist.exchange_and_merge(eng, rk.fresh(maps.n_loci, maps.n_haplotypes),
                                           rk.fresh(maps.n_loci, maps.n_haplotypes, multisample=True), root=0, finalize_ranges=per_range)
        sizes, n_ecs = None, 0
        if rank == 0:
            sizes = merged.b.finalize()
            n_ecs = sizes["n_ecs"]
        ecdist.exchange_multisample(eng, merged, n_ecs, root=0)
        tot = torch.tensor([n_all, n_valid], dtype=torch.int64, device=rk.wire)
        tdist.all_reduce(tot)
        n_all, n_valid = (int(x) for x in tot.cpu().tolist())
        range_len = None
        if track:
            mn, mx = b.export_range_minmax()
            mn, mx = np.minimum(mn.astype(np.int64), host_min), np.maximum(mx.astype(np.int64), host_max)
            range_len = ecdist.reduce_ranges(mn.astype(np.int32), mx.astype(np.int32), device=rk.wire)
        if rank == 0:
            _log_counts(maps, n_valid, sizes, len(names))
            f = _filter(merged.b, len(names), minimum_count)
            rk.result = _finish(maps, names, sizes, f, range_len, ec_filename, emase_filename, range_filename, rk.dev_index, n_all, n_valid,
                                start_time)


def convert(bam_filename, ec_filename, emase_filename, num_chunks=0, minimum_count=-1, number_processes=-1,
            temp_dir=None, range_filename=None, target_filename=None, best_strata=None, collapse_umis=False):
    """Same arguments as the reference (``bam_utils_multisample.py:357``); ``bam_filename`` is a directory."""
    if collapse_umis and umi_refusal(True, range_filename):
        raise CollapseUmisError(umi_refusal(True, range_filename))
    if os.path.isfile(bam_filename):
        LOG.error('bam file must be a directory')
        return None
    bam_files = sorted(glob.glob(os.path.join(bam_filename, "*.bam")))
    if len(bam_files) == 0:
        LOG.error('No bam files found in directory: {}'.format(bam_filename))
        return None
    return convert_files(bam_files, ec_filename, emase_filename, minimum_count, range_filename, target_filename, best_strata=best_strata,
                         collapse_umis=collapse_umis)
