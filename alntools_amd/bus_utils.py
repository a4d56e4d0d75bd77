# -*- coding: utf-8 -*-
"""``alntools bus2ec``: a multisample ``.bin`` from a ``kallisto bus`` output directory -- ``output.bus``, ``matrix.ec`` and
``transcripts.txt`` -- by bustools ``count``'s rule for EC matrices ("bus2ec").

The host reads the three files, checks the header, ``matrix.ec`` (parsed with numpy, no Python loop per line), the names and the
lengths; the records -- the bulk of the bytes -- go to the GPU as they lie in the file (``ecb_bus.molecules``): sorted, collapsed into
molecules, intersected where a molecule was seen in several ECs, and turned into rows and cell counts there.  The rows then go through
``ecb.combine`` as one part (equal keys become one EC) and ``ecb.select`` (the cell threshold ``-m``), and ``bin_utils.write_bin`` writes
the result.  The layouts are the ones the bustools documentation gives; no file here was checked against a bustools binary.

``-w/--whitelist FILE`` puts bustools ``correct``'s step in front: the records' barcodes are snapped onto the whitelist on the GPU
(``ecb_bus_correct.correct``) before anything else sees them.  ``alntools buscorrect`` (:func:`correct_file`) writes the corrected records
behind the input's header instead, for users who go on with other tools.
"""
from __future__ import annotations

import os
import re
import struct
import time

import numpy as np

from . import bin_utils, salmon_utils, utils

LOG = utils.get_logger()

MAGIC = b"BUS\0"
RECORD_BYTES = 32
MAX_RECORDS = 1 << 30            # radix_sort_pairs64's limit (include/ecb_bus.h)
BASES = "ACGT"
_CODE = {c: i for i, c in enumerate(BASES)}


def encode(seq):
    """The 2-bit value of a barcode or UMI (A=0, C=1, G=2, T=3, the first base in the most significant used bits); ValueError for a letter
    outside ACGT or more than 32 bases."""
    if len(seq) > 32:
        raise ValueError("{!r} has more than 32 bases".format(seq))
    v = 0
    for c in seq:
        if c not in _CODE:
            raise ValueError("{!r} has a letter outside ACGT".format(seq))
        v = v << 2 | _CODE[c]
    return v


def decode(value, length):
    """The ``length`` bases of a 2-bit value."""
    value = int(value)
    return "".join(BASES[(value >> (2 * (length - 1 - k))) & 3] for k in range(length))


class BusHeader(object):
    """``output.bus``'s header: the barcode and UMI lengths, where the records start, and their number."""

    def __init__(self, bclen, umilen, offset, n_records):
        self.bclen, self.umilen, self.offset, self.n_records = bclen, umilen, offset, n_records


def read_header(path):
    """The header of ``path``; ValueError for a wrong magic or version, ``bclen`` or ``umilen`` outside 1 .. 32, a size that is not
    header + 32 n, no records, or 2^30 records or more."""
    size = os.path.getsize(path)
    with open(path, 'rb') as fh:
        head = fh.read(20)
    if len(head) < 20 or head[:4] != MAGIC:
        raise ValueError("{}: not a BUS file (the first four bytes are not 'BUS\\0')".format(path))
    version, bclen, umilen, tlen = struct.unpack('<4I', head[4:])
    if version != 1:
        raise ValueError("{}: BUS version {}; only version 1 is read".format(path, version))
    if not 1 <= bclen <= 32:
        raise ValueError("{}: a barcode length of {} (1 .. 32)".format(path, bclen))
    if not 1 <= umilen <= 32:
        raise ValueError("{}: a UMI length of {} (1 .. 32)".format(path, umilen))
    offset = 20 + tlen
    if size < offset or (size - offset) % RECORD_BYTES:
        raise ValueError("{}: {} bytes are not a header of {} bytes and whole records of {}".format(path, size, offset, RECORD_BYTES))
    n = (size - offset) // RECORD_BYTES
    if n == 0:
        raise ValueError("{}: no records".format(path))
    if n >= MAX_RECORDS:
        raise ValueError("{}: {:,} records; 2^30 or more are beyond one sort".format(path, n))
    return BusHeader(bclen, umilen, offset, n)


def read_records(path, hdr):
    """The records as they lie in the file: uint8 ``[n, 32]``."""
    return np.fromfile(path, dtype=np.uint8, offset=hdr.offset).reshape(-1, RECORD_BYTES)


def read_transcripts(path):
    """``transcripts.txt``: one target name per line."""
    with open(path) as fh:
        return [ln.rstrip('\r\n') for ln in fh]


def parse_matrix_ec(path, n_targets):
    """``matrix.ec`` (line i is ``i<TAB>t1,t2,...``) -> (ec_ptr uint32 [E + 1], ec_targets uint32), vectorised.  ValueError with the file
    and line for a byte that does not belong, a line that is not one number, a tab and a comma-separated list, a line number out of
    sequence, a target id at or beyond ``n_targets`` or ids that are not strictly ascending."""
    with open(path, 'rb') as fh:
        data = fh.read()
    if data and not data.endswith(b"\n"):
        data += b"\n"
    buf = np.frombuffer(data, dtype=np.uint8)
    if not len(buf):
        raise ValueError("{}: no lines".format(path))

    def refuse(at, what):
        raise ValueError("{} line {}: {}".format(path, int(np.count_nonzero(buf[:int(at)] == 10)) + 1, what))
    digit = (buf >= 48) & (buf <= 57)
    sep = (buf == 9) | (buf == 44) | (buf == 10)
    bad = np.flatnonzero(~(digit | sep))
    if len(bad):
        refuse(bad[0], "a byte other than a digit, tab, comma or line end")
    prev_digit = np.concatenate(([False], digit[:-1]))
    next_digit = np.concatenate((digit[1:], [False]))
    # a separator stands after a digit; a tab or comma also before one
    bad = np.flatnonzero(sep & (~prev_digit | ((buf != 10) & ~next_digit)))
    if len(bad):
        refuse(bad[0], "an empty field")
    starts = np.flatnonzero(digit & ~prev_digit)
    ends = np.flatnonzero(digit & ~next_digit)                  # (the last digit of every number)
    if len(starts) and int((ends - starts).max()) >= 10:
        refuse(starts[int(np.argmax(ends - starts))], "a number of more than 10 digits")
    run_end = np.repeat(ends, ends - starts + 1)
    where = np.flatnonzero(digit)
    values = np.add.reduceat((buf[where] - 48).astype(np.int64) * 10 ** (run_end - where).astype(np.int64), np.cumsum(ends - starts + 1) - (ends - starts + 1))
    after = buf[ends + 1]                                        # the separator behind every number
    newline = np.flatnonzero(buf == 10)
    first = np.concatenate(([0], np.flatnonzero(after == 10)[:-1] + 1))      # the first number of every line
    is_first = np.zeros(len(starts), dtype=bool)
    is_first[first] = True
    bad = np.flatnonzero(is_first != (after == 9))               # a tab behind the first number of a line, and nowhere else
    if len(bad):
        refuse(starts[bad[0]], "not <number><TAB><id>,<id>,...")
    n_lines = len(newline)
    bad = np.flatnonzero(values[first] != np.arange(n_lines))
    if len(bad):
        refuse(starts[first[bad[0]]], "line number {} out of sequence (expected {})".format(int(values[first[bad[0]]]), int(bad[0])))
    ids = values[~is_first]
    id_at = starts[~is_first]
    bad = np.flatnonzero(ids >= n_targets)
    if len(bad):
        refuse(id_at[bad[0]], "target id {} at or beyond the {} names of transcripts.txt".format(int(ids[bad[0]]), n_targets))
    per_line = np.diff(np.concatenate((first, [len(starts)]))) - 1
    ptr = np.concatenate(([0], np.cumsum(per_line)))
    inner = np.ones(len(ids), dtype=bool)
    inner[ptr[:-1][per_line > 0]] = False                         # (not the first id of a line)
    bad = np.flatnonzero(inner[1:] & (ids[1:] <= ids[:-1])) + 1 if len(ids) > 1 else []
    if len(bad):
        refuse(id_at[bad[0]], "target ids not strictly ascending")
    if ptr[-1] >= 1 << 32 or n_lines >= 1 << 31:
        raise ValueError("{}: beyond 32 bits".format(path))
    return ptr.astype(np.uint32), ids.astype(np.uint32)


def number_bus_targets(names, extra_transcripts=(), haplotype=None, path='transcripts.txt'):
    """``salmon_utils.number_targets`` for ``transcripts.txt`` (line numbers from 1); with ``haplotype``, every name is a transcript as it
    stands and ``haplotype`` the single haplotype."""
    seen = {}
    for i, name in enumerate(names):
        if haplotype is None and len(name.split('_')) != 2:
            raise ValueError("{} line {}: target name {!r} is not <transcript>_<haplotype> (exactly one '_')".format(path, i + 1, name))
        if name in seen:
            raise ValueError("{} line {}: target name {!r} is listed twice (first on line {})".format(path, i + 1, name, seen[name] + 1))
        seen[name] = i
    if haplotype is None:
        return salmon_utils.number_targets(names, extra_transcripts, path)
    transcripts = list(names) + [t for t in dict.fromkeys(extra_transcripts) if t not in seen]
    return transcripts, [haplotype], np.arange(len(names), dtype=np.uint32), np.zeros(len(names), dtype=np.uint32)


def read_names(path, bclen):
    """``--names FILE``: lines of ``barcode<TAB>name`` -> (values uint64, names), in the file's order.  ValueError with the file and line for
    a line that is not two fields, a barcode of another length than ``bclen``, a letter outside ACGT, a barcode or a name listed twice."""
    values, names, seen_b, seen_n = [], [], {}, {}
    with open(path) as fh:
        for k, line in enumerate(fh):
            where = "{} line {}".format(path, k + 1)
            item = line.rstrip('\r\n').split('\t')
            if len(item) != 2 or not item[1]:
                raise ValueError("{}: not <barcode><TAB><name>".format(where))
            bc, name = item
            if len(bc) != bclen:
                raise ValueError("{}: barcode {!r} has {} bases; the BUS file's have {}".format(where, bc, len(bc), bclen))
            try:
                v = encode(bc)
            except ValueError as e:
                raise ValueError("{}: barcode {}".format(where, e))
            if v in seen_b:
                raise ValueError("{}: barcode {!r} is listed twice (first on line {})".format(where, bc, seen_b[v] + 1))
            if name in seen_n:
                raise ValueError("{}: name {!r} is listed twice (first on line {})".format(where, name, seen_n[name] + 1))
            seen_b[v], seen_n[name] = k, k
            values.append(v)
            names.append(name)
    return np.array(values, dtype=np.uint64), names


def read_lengths(path, names):
    """``-l LENGTHS``: ``name<TAB>length`` per target name, under ``salmon_utils.read_lengths``' rules (truncated toward zero; ValueError for a
    name that is not a target, a name listed twice, a missing or non-numeric length, one beyond int32, or a target with no line)."""
    index = {n: i for i, n in enumerate(names)}
    lengths = np.zeros(len(names), dtype=np.int64)
    have = np.zeros(len(names), dtype=bool)
    with open(path) as fh:
        for k, line in enumerate(fh):
            item = line.rstrip().split('\t')
            where = "{} line {}".format(path, k + 1)
            i = index.get(item[0])
            if i is None:
                raise ValueError("{}: target {!r} is not in transcripts.txt".format(where, item[0]))
            if have[i]:
                raise ValueError("{}: target {!r} is listed twice".format(where, item[0]))
            if len(item) < 2:
                raise ValueError("{}: no length column".format(where))
            try:
                v = float(item[1])
            except ValueError:
                raise ValueError("{}: length {!r} is not a number".format(where, item[1]))
            if not np.isfinite(v) or not -2.0 ** 31 < v < 2.0 ** 31:
                raise ValueError("{}: length {!r} is beyond int32".format(where, item[1]))
            lengths[i], have[i] = int(v), True
    if not have.all():
        raise ValueError("{}: target {!r} of transcripts.txt has no line".format(path, names[int(np.flatnonzero(~have)[0])]))
    return lengths


def read_whitelist(path, bclen):
    """``-w FILE``: one barcode per line, plain or gzipped (a name ending in ``.gz``) -> uint64, sorted ascending; parsed with numpy, no
    Python loop per line (a kit's list has millions).  ``\\r\\n`` line ends and a missing final line end are taken.  ValueError with the
    file and line for a barcode of another length than ``bclen`` (an empty line is one), a letter outside ACGT, a barcode listed twice
    (naming the first line too), and for an empty file."""
    if path.endswith(".gz"):
        import gzip
        with gzip.open(path, 'rb') as fh:
            data = fh.read()
    else:
        with open(path, 'rb') as fh:
            data = fh.read()
    if not data:
        raise ValueError("{}: no barcodes (the file is empty)".format(path))
    if not data.endswith(b"\n"):
        data += b"\n"
    buf = np.frombuffer(data, dtype=np.uint8)
    cr = np.flatnonzero((buf[:-1] == 13) & (buf[1:] == 10))
    if len(cr):
        buf = np.delete(buf, cr)
    ends = np.flatnonzero(buf == 10)
    starts = np.concatenate(([0], ends[:-1] + 1))

    def text(line):
        return bytes(buf[starts[line]:ends[line]]).decode('latin-1')
    bad = np.flatnonzero(ends - starts != bclen)
    if len(bad):
        k = int(bad[0])
        raise ValueError("{} line {}: barcode {!r} has {} bases; the BUS file's have {}".format(path, k + 1, text(k), int(ends[k] - starts[k]), bclen))
    code = np.full(256, 255, dtype=np.uint8)
    code[np.frombuffer(BASES.encode(), dtype=np.uint8)] = np.arange(4, dtype=np.uint8)
    codes = code[buf.reshape(len(ends), bclen + 1)[:, :bclen]]
    bad = np.flatnonzero((codes == 255).any(axis=1))
    if len(bad):
        raise ValueError("{} line {}: barcode {!r} has a letter outside ACGT".format(path, int(bad[0]) + 1, text(int(bad[0]))))
    values = np.zeros(len(ends), dtype=np.uint64)
    for k in range(bclen):                                       # (a pass per base, not per line)
        values = (values << np.uint64(2)) | codes[:, k]
    order = np.argsort(values, kind='stable')
    out = values[order]
    dup = np.flatnonzero(out[1:] == out[:-1])
    if len(dup):
        second = int(order[dup + 1].min())
        first = int(np.flatnonzero(values == values[second])[0])
        raise ValueError("{} line {}: barcode {!r} is listed twice (first on line {})".format(path, second + 1, text(second), first + 1))
    return out


def correct_records(records, bclen, whitelist_file, bus_path, device=0):
    """The records with their barcodes snapped onto the whitelist of ``whitelist_file`` on the GPU (``ecb_bus_correct.correct``) -> (the
    records kept, uint8 ``[n_out, 32]``, (exact, corrected, without a candidate, ambiguous)).  ValueError naming the file and the record
    or line for what the library refuses, and when no record is left."""
    from . import ecb, ecb_bus, ecb_bus_correct
    whitelist = read_whitelist(whitelist_file, bclen)
    LOG.info("Correcting the barcodes against the {:,} of {} on the GPU".format(len(whitelist), whitelist_file))
    try:
        out, _status, sizes = ecb_bus_correct.correct(records, bclen, whitelist, device=device)
    except ecb_bus_correct.WhitelistFormatError as e:
        raise ValueError("{}: {}".format(whitelist_file, str(e.args[0]).split("bus: ", 1)[-1]))
    except ecb_bus.BusFormatError as e:
        raise ValueError("{} record {}: {}".format(bus_path, e.index, re.split(r"record \d+: ", str(e.args[0]), maxsplit=1)[-1]))
    except ecb.EcbError as e:
        raise ValueError("{}: {}".format(bus_path, e.args[0]))
    if not len(out):
        raise ValueError("{}: no record has a barcode on or next to the whitelist".format(bus_path))
    return out, sizes


STATS = ("records", "molecules", "molecules_in_several_ecs", "molecules_discarded", "new_ecs", "cells", "cells_kept")
WHITELIST_STATS = ("barcodes_exact", "barcodes_corrected", "barcodes_without_candidate", "barcodes_ambiguous")      # ecb_bus_correct's sizes, in order


def stats_text(stats):
    """``--stats FILE``: one ``name<TAB>value`` line for each of :data:`STATS` and, after a whitelist correction (``-w``), for each of
    :data:`WHITELIST_STATS`."""
    keys = STATS + (WHITELIST_STATS if all(k in stats for k in WHITELIST_STATS) else ())
    return "".join("{}\t{}\n".format(k, int(stats[k])) for k in keys)


def bus_matrices(bus_dir, no_umi=False, mincount=1000, names_file=None, lengths_file=None, haplotype=None, target_filename=None, want_stats=False,
                 device=0, whitelist_file=None):
    """Everything of :func:`convert` but the writing: -> (:class:`bin_utils.ECMatrices`, stats dict).  Raises ValueError (with the file and
    the line or record) for every input it refuses.  ``whitelist_file``: the records' barcodes are corrected against it first
    (:func:`correct_records`); everything after sees the corrected records, the keep list of ``names_file`` included."""
    from . import ecb, ecb_bus
    bus_path, ec_path, tx_path = (os.path.join(bus_dir, f) for f in ("output.bus", "matrix.ec", "transcripts.txt"))
    hdr = read_header(bus_path)
    if not no_umi and hdr.umilen > ecb_bus.MAX_UMILEN:
        raise ValueError("{}: a UMI length of {}; the sort keys hold {} (--no-umi takes any)".format(bus_path, hdr.umilen, ecb_bus.MAX_UMILEN))
    names = read_transcripts(tx_path)
    extra = salmon_utils.read_targets(target_filename) if target_filename is not None else []
    transcripts, haplotypes, col, hap = number_bus_targets(names, extra, haplotype, tx_path)
    if not names:
        raise ValueError("{}: no targets".format(tx_path))
    if len(haplotypes) > 31:
        raise ValueError("{}: {} haplotypes; a .bin holds at most 31".format(tx_path, len(haplotypes)))
    lengths = np.zeros((len(transcripts), len(haplotypes)), dtype=np.int64)
    if lengths_file is not None:
        lengths[col, hap] = read_lengths(lengths_file, names)
    LOG.info("Parsing {}".format(ec_path))
    ec_ptr, ec_targets = parse_matrix_ec(ec_path, len(names))
    keep = order = snames = None
    if names_file is not None:
        values, snames = read_names(names_file, hdr.bclen)
        order = np.argsort(values, kind='stable')
        keep = values[order]
    LOG.info("Reading {:,} records of {}".format(hdr.n_records, bus_path))
    records = read_records(bus_path, hdr)
    corrected = None
    if whitelist_file is not None:
        records, corrected = correct_records(records, hdr.bclen, whitelist_file, bus_path, device=device)
    LOG.info("Collapsing the records into molecules and rows on the GPU")
    try:
        barcodes, A, N, row_line, sizes = ecb_bus.molecules(records, hdr.bclen, hdr.umilen, ec_ptr, ec_targets, col, hap, len(transcripts),
                                                            len(haplotypes), keep=keep, no_umi=no_umi, device=device)
    except ecb_bus.BusFormatError as e:
        text = re.split(r"(?:record|line) \d+: ", str(e.args[0]), maxsplit=1)[-1]
        if e.what == "record":
            raise ValueError("{} record {}: {}".format(bus_path, e.index, text))
        raise ValueError("{} line {}: {}".format(ec_path, e.index + 1, text))
    except ecb.EcbError as e:
        raise ValueError("{}: {}".format(bus_path, e.args[0]))
    n_cells = len(barcodes)
    if n_cells == 0:
        raise ValueError("no sample left")
    if snames is None:
        snames = [decode(b, hdr.bclen) for b in barcodes]
        sample_map = None
    else:
        sample_map = order[np.searchsorted(keep, barcodes)].astype(np.uint32)
    part = dict(indptrA=A[0], indicesA=A[1], dataA=A[2], indptrN=N[0], indicesN=N[1], dataN=N[2], n_loci=len(transcripts), target_map=None,
                sample_map=np.arange(n_cells, dtype=np.uint32) if sample_map is None else sample_map)
    try:
        combined = ecb.combine([part], len(transcripts), len(haplotypes), len(snames), device=device)
        A_N, kept = ecb.select(*combined, len(transcripts), len(haplotypes), row_class=0, sample_keep=None, min_count=mincount, device=device)
        new_ecs = 0
        if want_stats:
            r1 = int(np.count_nonzero(row_line >= 0))
            lines = dict(part, indptrA=A[0][:r1 + 1], indicesA=A[1][:A[0][r1]], dataA=A[2][:A[0][r1]], indptrN=np.zeros(n_cells + 1, dtype=np.int32),
                         indicesN=np.zeros(0, dtype=np.int32), dataN=np.zeros(0, dtype=np.int32))
            new_ecs = len(combined[0]) - len(ecb.combine([lines], len(transcripts), len(haplotypes), len(snames), device=device)[0])
    except ecb.EcbError as e:
        raise ValueError("{}: {}".format(bus_path, e.args[0]))
    m = bin_utils.ECMatrices(haplotypes, transcripts, lengths, [s for s, k in zip(snames, kept) if k], *A_N)
    stats = dict(records=hdr.n_records, molecules=sizes[4], molecules_in_several_ecs=sizes[5], molecules_discarded=sizes[6], new_ecs=new_ecs,
                 cells=n_cells, cells_kept=m.num_samples)
    if corrected is not None:
        stats.update(zip(WHITELIST_STATS, corrected))
    if m.num_samples == 0:
        raise ValueError("no sample left")
    return m, stats


def convert(bus_dir, ec_filename, no_umi=False, mincount=1000, names_file=None, lengths_file=None, haplotype=None, target_filename=None,
            stats_file=None, device=0, whitelist_file=None):
    """``alntools bus2ec``: the multisample ``.bin`` of a ``kallisto bus`` output directory, written with ``bin_utils.write_bin``.  Any
    failure is logged as ``Error: ...``, no file is left behind, and the exception is raised again (the command line exits with status 1)."""
    LOG.debug('-------------------------------------------')
    LOG.debug('Parameters:')
    LOG.debug('  BUS directory: {}'.format(bus_dir))
    LOG.debug('  EC file: {}'.format(ec_filename))
    LOG.debug('  UMIs: {}'.format("ignored" if no_umi else "collapsed"))
    LOG.debug('  Minimum count: {}'.format(mincount))
    LOG.debug('  Names file: {}'.format(names_file))
    LOG.debug('  Lengths file: {}'.format(lengths_file))
    LOG.debug('  Haplotype: {}'.format(haplotype))
    LOG.debug('  Target file: {}'.format(target_filename))
    LOG.debug('  Whitelist: {}'.format(whitelist_file))
    LOG.debug('-------------------------------------------')
    written = []
    with bin_utils.command(bin_utils.RAISE, written=written):
        time0 = time.time()
        m, stats = bus_matrices(bus_dir, no_umi=no_umi, mincount=mincount, names_file=names_file, lengths_file=lengths_file, haplotype=haplotype,
                                target_filename=target_filename, want_stats=stats_file is not None, device=device, whitelist_file=whitelist_file)
        LOG.info("{} parsed in {}".format(bus_dir, utils.format_time(time0, time.time())))
        time1 = time.time()
        bin_utils.log_saving("Converting and storing to {}".format(ec_filename), m,
                             "Number of samples: {:,} (of {:,} cells)".format(m.num_samples, stats["cells"]),
                             "Number of equivalence classes: {:,}".format(m.num_reads), samples=None)
        if stats_file is not None:
            with open(stats_file, 'w') as fh:
                written.append(stats_file)
                fh.write(stats_text(stats))
        bin_utils.write_bin(ec_filename, m)
        LOG.info("{} created in {}".format(ec_filename, utils.format_time(time1, time.time())))


def correct_file(bus_file, out_file, whitelist_file, stats_file=None, device=0):
    """``alntools buscorrect``: what ``bustools correct`` writes -- the header bytes of ``bus_file`` as they are, text included, then the
    records whose barcode is on the whitelist or one base from exactly one of its barcodes, that barcode in place, in the file's order.
    ``stats_file``: the number of records and :data:`WHITELIST_STATS`.  Failures as in :func:`convert`."""
    written = []
    with bin_utils.command(bin_utils.RAISE, written=written):
        time0 = time.time()
        if os.path.exists(out_file) and os.path.samefile(bus_file, out_file):
            raise ValueError("{}: the output is the input".format(out_file))
        hdr = read_header(bus_file)
        with open(bus_file, 'rb') as fh:
            head = fh.read(hdr.offset)
        LOG.info("Reading {:,} records of {}".format(hdr.n_records, bus_file))
        out, sizes = correct_records(read_records(bus_file, hdr), hdr.bclen, whitelist_file, bus_file, device=device)
        LOG.info("Storing {:,} of {:,} records to {}".format(len(out), hdr.n_records, out_file))
        if stats_file is not None:
            with open(stats_file, 'w') as fh:
                written.append(stats_file)
                fh.write("records\t{}\n".format(hdr.n_records) + "".join("{}\t{}\n".format(k, int(v)) for k, v in zip(WHITELIST_STATS, sizes)))
        with open(out_file, 'wb') as fh:
            written.append(out_file)
            fh.write(head)
            np.ascontiguousarray(out).tofile(fh)
        LOG.info("{} created in {}".format(out_file, utils.format_time(time0, time.time())))
