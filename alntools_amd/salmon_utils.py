# -*- coding: utf-8 -*-
"""``alntools salmon2ec``: a ``.bin`` from a salmon run's equivalence classes (the reference's ``salmon_utils.parse_salmon_ec`` +
``convert``, ``alntools/salmon_utils.py:31-127, 231-248``).

The host reads the file and checks the header, ``quant.sf`` and the ``-t`` file; the EC section -- the bulk of the bytes -- is
parsed, checked and turned into CSR A and N on the GPU (``ecb.salmon_ecs``).  What the reference does, and keeps:

* header: line 1 = T, line 2 = E, then T target names, each ``name.rstrip().split('_')`` into exactly (transcript, haplotype);
* transcripts (the columns) and haplotypes are numbered by first appearance in the header; ``-t`` appends the first tab-column names
  of its file (``np.loadtxt``: ``#`` comments and blank lines skipped) that are not there yet;
* lengths: ``quant.sf`` column 3 (EffectiveLength), truncated toward zero; a (transcript, haplotype) without a target gets 0;
* A[e, t] = sum of 2^h over the targets of transcript t in EC line e; N = the ECs with a non-zero count.

Where the reference crashes or writes a ``.bin`` that is silently wrong, this refuses: a repeated header name or
``quant.sf`` name, k that differs from the number of target ids, a target id twice in one line, a number of EC lines other than E,
more than 31 haplotypes, lengths beyond int32.  ``aux_info/eq_classes.txt.gz`` is read when the plain file is not there.
"""
from __future__ import annotations

import gzip
import os
import time

import numpy as np

from . import bin_utils, utils

LOG = utils.get_logger()


def eq_classes_path(salmon_dir):
    """``aux_info/eq_classes.txt``, or ``eq_classes.txt.gz`` when only that exists (what current salmon releases write)."""
    plain = os.path.join(salmon_dir, 'aux_info', 'eq_classes.txt')
    if os.path.exists(plain) or not os.path.exists(plain + '.gz'):
        return plain
    return plain + '.gz'


def read_eq_classes(path):
    """The file's bytes (decompressed when it ends in ``.gz``)."""
    with open(path, 'rb') as fh:
        data = fh.read()
    return gzip.decompress(data) if path.endswith('.gz') else data


def _line_ends(buf, count):
    """Offsets of the first ``count`` line ends of ``buf`` (uint8), fewer when it has fewer; only the prefix that holds them is read."""
    ends, start, chunk = [], 0, 1 << 20
    while len(ends) < count and start < len(buf):
        nl = np.flatnonzero(buf[start:start + chunk] == 10) + start
        ends.extend(nl[:count - len(ends)].tolist())
        start += chunk
        chunk *= 2
    return ends


class SalmonHeader(object):
    """The header of ``eq_classes.txt``: T, E, the target names, where the EC section starts, and the number of header lines."""

    def __init__(self, n_targets, n_ecs, names, ec_offset):
        self.n_targets, self.n_ecs, self.names, self.ec_offset = n_targets, n_ecs, names, ec_offset
        self.n_lines = 2 + n_targets


def parse_header(data, path='eq_classes.txt'):
    """T, E and the T names of ``data`` (the file's bytes); raises ValueError with the line number when the header is malformed."""
    buf = np.frombuffer(data, dtype=np.uint8)
    first = _line_ends(buf, 2)
    if len(first) < 2:
        raise ValueError("{}: the header ends before the number of ECs (line 2)".format(path))
    counts = []
    for k, (a, b) in enumerate(((0, first[0]), (first[0] + 1, first[1]))):
        line = data[a:b]
        try:
            counts.append(int(line))
        except ValueError:
            raise ValueError("{} line {}: the number of {} is not an integer: {!r}".format(
                path, k + 1, ("targets", "ECs")[k], line.decode('utf-8', 'replace')))
        if counts[-1] < 0:
            raise ValueError("{} line {}: a negative count {}".format(path, k + 1, counts[-1]))
    T, E = counts
    ends = _line_ends(buf, 2 + T)
    if len(ends) == 2 + T:
        ec_offset = ends[-1] + 1
        body = data[first[1] + 1:ends[-1]]
    elif len(ends) == 1 + T and len(data) > ends[-1] + 1:          # (the last name ends the file)
        ec_offset = len(data)
        body = data[first[1] + 1:]
    else:
        raise ValueError("{}: the header lists {} target names, fewer than T = {}".format(path, max(len(ends) - 2, 0), T))
    names = body.decode('utf-8').split('\n') if T else []
    return SalmonHeader(T, E, [n.rstrip() for n in names], ec_offset)


def number_targets(names, extra_transcripts=(), path='eq_classes.txt'):
    """(transcripts, haplotypes, target_col, target_hap): both name lists in first-seen order (``extra_transcripts`` appended to the
    transcripts where new), and each target's column and haplotype.  Raises ValueError for a name that is not ``transcript_haplotype``
    or that is listed twice (the reference crashes on both)."""
    tid, hid, seen = {}, {}, {}
    col = np.empty(len(names), dtype=np.uint32)
    hap = np.empty(len(names), dtype=np.uint32)
    for i, name in enumerate(names):
        parts = name.split('_')
        if len(parts) != 2:
            raise ValueError("{} line {}: target name {!r} is not <transcript>_<haplotype> (exactly one '_')".format(path, 3 + i, name))
        if name in seen:
            raise ValueError("{} line {}: target name {!r} is listed twice (first on line {})".format(path, 3 + i, name, 3 + seen[name]))
        seen[name] = i
        t, h = parts
        col[i] = tid.setdefault(t, len(tid))
        hap[i] = hid.setdefault(h, len(hid))
    for t in extra_transcripts:
        tid.setdefault(t, len(tid))
    return list(tid), list(hid), col, hap


def read_targets(target_filename):
    """The first tab-column of a target file, as the reference reads it (``np.loadtxt(..., dtype=str, delimiter='\\t', usecols=(0,))``)."""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return [str(t) for t in np.loadtxt(target_filename, dtype=str, delimiter='\t', usecols=(0,), ndmin=1)]


def read_lengths(quant_file, names):
    """Effective lengths (``quant.sf`` column 3) of the header's targets, truncated toward zero, as int64.  Raises ValueError for a
    name that is not in the header, a name listed twice, a missing or non-numeric column, a length beyond int32, or a header target
    with no line."""
    index = {n: i for i, n in enumerate(names)}
    lengths = np.full(len(names), -1, dtype=np.int64)
    have = np.zeros(len(names), dtype=bool)
    with open(quant_file) as qfh:
        qfh.readline()
        for k, curline in enumerate(qfh):
            item = curline.rstrip().split('\t')
            where = "{} line {}".format(quant_file, k + 2)
            i = index.get(item[0])
            if i is None:
                raise ValueError("{}: target {!r} is not in the eq_classes header".format(where, item[0]))
            if have[i]:
                raise ValueError("{}: target {!r} is listed twice".format(where, item[0]))
            if len(item) < 3:
                raise ValueError("{}: no EffectiveLength column".format(where))
            try:
                v = float(item[2])
            except ValueError:
                raise ValueError("{}: EffectiveLength {!r} is not a number".format(where, item[2]))
            if not np.isfinite(v) or not -2.0 ** 31 < v < 2.0 ** 31:
                raise ValueError("{}: EffectiveLength {!r} is beyond int32".format(where, item[2]))
            lengths[i], have[i] = int(v), True
    if not have.all():
        missing = names[int(np.flatnonzero(~have)[0])]
        raise ValueError("{}: target {!r} of the eq_classes header has no line".format(quant_file, missing))
    return lengths


def parse_salmon_ec(salmon_dir, target_filename=None, device=0):
    """The reference's ``parse_salmon_ec``: -> (transcripts, haplotypes, lengths[T x H], (indptrA, indicesA, dataA), (indptrN, indicesN,
    dataN)), A and N built on the GPU.  Raises ValueError (with the file and line) for every input it refuses."""
    from . import ecb
    path = eq_classes_path(salmon_dir)
    quant_file = os.path.join(salmon_dir, 'quant.sf')
    extra = read_targets(target_filename) if target_filename is not None else []
    LOG.info("Parsing {}".format(path))
    data = read_eq_classes(path)
    hdr = parse_header(data, path)
    transcripts, haplotypes, col, hap = number_targets(hdr.names, extra, path)
    if not transcripts or not haplotypes:
        raise ValueError("{}: no targets".format(path))
    if len(haplotypes) > 31:
        raise ValueError("{}: {} haplotypes; a .bin holds at most 31".format(path, len(haplotypes)))
    LOG.info('Reading in the effective transcript lengths from {}'.format(quant_file))
    eff = read_lengths(quant_file, hdr.names)
    lengths = np.zeros((len(transcripts), len(haplotypes)), dtype=np.int64)
    lengths[col, hap] = eff
    LOG.info('Creating EC alignment incidence matrix')
    section = np.frombuffer(data, dtype=np.uint8, offset=hdr.ec_offset) if hdr.ec_offset < len(data) else np.zeros(0, dtype=np.uint8)
    try:
        ip, ix, da, nix, nda = ecb.salmon_ecs(section, hdr.n_ecs, col, hap, len(transcripts), len(haplotypes), device=device)
    except ecb.SalmonFormatError as e:
        raise ValueError("{} line {}: {}".format(path, hdr.n_lines + 1 + e.line, ecb.SALMON_REASONS.get(e.reason, e.args[0])))
    LOG.info('Creating EC count matrix')
    return transcripts, haplotypes, lengths, (ip, ix, da), (np.array([0, len(nix)], dtype=np.int32), nix, nda)


def convert(salmon_dir, ec_filename, sample='NA', target_filename=None, device=0):
    """``alntools salmon2ec``: the ``.bin`` of a salmon run's equivalence classes, written with ``bin_utils.ecsave2``.  Any failure is
    logged as ``Error: ...``, no file is left behind, and the exception is raised again (the command line exits with status 1)."""
    LOG.debug('-------------------------------------------')
    LOG.debug('Parameters:')
    LOG.debug('  SALMON directory: {}'.format(salmon_dir))
    LOG.debug('  EC file: {}'.format(ec_filename))
    LOG.debug('  Sample: {}'.format(sample))
    LOG.debug('  Target file: {}'.format(target_filename))
    LOG.debug('-------------------------------------------')
    with bin_utils.command(bin_utils.RAISE):
        time0 = time.time()
        transcripts, haplotypes, lengths, A, N = parse_salmon_ec(salmon_dir, target_filename, device=device)
        LOG.info("{} parsed in {}".format(ec_filename, utils.format_time(time0, time.time())))
        time1 = time.time()
        m = bin_utils.ECMatrices(haplotypes, transcripts, lengths, [sample], *A, *N)
        bin_utils.log_saving("Converting and storing to {}".format(ec_filename), m, "Number of equivalence classes: {:,}".format(m.num_reads),
                             samples=None)
        bin_utils.write_bin(ec_filename, m)
        LOG.info("{} created in {}".format(ec_filename, utils.format_time(time1, time.time())))
