# -*- coding: utf-8 -*-
"""EC ``.bin`` format 2, byte-exact with the reference's ``bin_utils.ecsave2`` / ``ecload``
(``alntools/bin_utils.py:105-277, 32-102``).

The reference packs every array with ``struct.pack('<Ni', *array)`` (one Python int per
element); here the same little-endian int32 bytes come from ``ndarray.astype('<i4').tobytes()``.
Layout: ``2``; ``H`` then H x (len, utf-8 name); ``T`` then T x (len, name, H lengths);
``S`` then S x (len, name); A as CSR (``len(indptr)``, ``nnz``, indptr, indices = locus,
data = haplotype bitmask); N as CSC (``len(indptr)``, ``nnz``, indptr, indices = EC, data = count).
"""
from __future__ import annotations

import contextlib
import os
import time
from struct import pack, unpack_from

import numpy as np

from . import utils

LOG = utils.get_logger()


class ECMatrices(object):
    """What ``ecsave2`` consumes and ``ecload`` returns: names, lengths, CSR A and CSC N.

    The slice of the reference's ``AlignmentPropertyMatrix`` (shape-constructed, finalized;
    ``AlignmentPropertyMatrix.py:148-171``, ``Sparse3DMatrix.py:189-193``) that the hot path fills.
    """

    def __init__(self, hname, lname, lengths, sname, indptrA, indicesA, dataA, indptrN, indicesN, dataN):
        self.hname, self.lname, self.sname = list(hname), list(lname), list(sname)
        self.lengths = np.asarray(lengths)
        self.indptrA, self.indicesA, self.dataA = (np.asarray(x, dtype=np.int32) for x in (indptrA, indicesA, dataA))
        self.indptrN, self.indicesN, self.dataN = (np.asarray(x, dtype=np.int32) for x in (indptrN, indicesN, dataN))

    num_haplotypes = property(lambda s: len(s.hname))
    num_loci = property(lambda s: len(s.lname))
    num_samples = property(lambda s: len(s.sname))
    num_reads = property(lambda s: len(s.indptrA) - 1)
    shape = property(lambda s: (len(s.lname), len(s.hname), len(s.indptrA) - 1))

    def haplotype_csc(self, h):
        """Per-haplotype CSC (E x T) incidence, as ``apm.data[h]`` after ``finalize()``."""
        from scipy.sparse import csr_matrix
        bit = ((self.dataA >> h) & 1).astype(np.float64)
        m = csr_matrix((bit, self.indicesA.copy(), self.indptrA.copy()), shape=(self.num_reads, self.num_loci))
        m.eliminate_zeros()
        return m.tocsc()


def _name(s):
    return pack('<i', len(s)) + pack('<{}s'.format(len(s)), s.encode('utf-8'))


def _i32(a):
    return np.ascontiguousarray(a).astype('<i4').tobytes()


def ecsave2_bytes(m):
    out = [pack('<i', 2), pack('<i', m.num_haplotypes)]
    out += [_name(h) for h in m.hname]
    out.append(pack('<i', m.num_loci))
    lens = np.asarray(m.lengths).astype(int)                       # bin_utils.py:153
    for t, name in enumerate(m.lname):
        out.append(_name(name))
        out.append(_i32(lens[t, :m.num_haplotypes]))
    out.append(pack('<i', m.num_samples))
    out += [_name(s) for s in m.sname]
    out += [pack('<i', len(m.indptrA)), pack('<i', len(m.indicesA)), _i32(m.indptrA), _i32(m.indicesA), _i32(m.dataA)]
    out += [pack('<i', len(m.indptrN)), pack('<i', len(m.indicesN)), _i32(m.indptrN), _i32(m.indicesN), _i32(m.dataN)]
    return b"".join(out)


def ecsave2(ec_filename, m):
    """Write ``m`` (:class:`ECMatrices`) as EC format 2 -- same bytes as the reference writer."""
    with open(ec_filename, 'wb') as f:
        f.write(ecsave2_bytes(m))


def write_bin(ec_filename, m):
    """``m`` as ``ec_filename``, whole or not at all: the bytes are made first, and a file that could not be finished is removed
    before the failure is raised again."""
    b = ecsave2_bytes(m)
    try:
        with open(ec_filename, 'wb') as fh:
            fh.write(b)
    except BaseException:
        if os.path.exists(ec_filename):
            os.remove(ec_filename)
        raise


#: what a command does with a failure, after its ``Error: ...`` line: raise it again -- a KeyError shown by its argument (``KEY``) or as
#: ``str()`` shows it (``RAISE``) -- or return normally, as the reference's commands do (``SWALLOW``)
KEY, RAISE, SWALLOW = "key", "raise", "swallow"


@contextlib.contextmanager
def command(failure, created=None, written=()):
    """The shell of a command: the clock, the closing ``<created> created in total time`` line (``created`` None: no such line) and,
    for a failure, the removal of the files in ``written`` -- the ones this run has opened so far, never another -- the ``Error: ...``
    line and what ``failure`` (``KEY``, ``RAISE`` or ``SWALLOW``) says happens then."""
    try:
        start_time = time.time()
        yield
        if created is not None:
            LOG.info("{} created in total time: {}".format(created, utils.format_time(start_time, time.time())))
    except Exception as e:
        for f in written:
            try:
                os.remove(f)
            except OSError:
                pass
        LOG.error("Error: {}".format(e.args[0] if failure == KEY and isinstance(e, KeyError) and e.args else str(e)))
        if failure != SWALLOW:
            raise


def log_saving(first, m, *rest, samples="Number of samples: {:,}"):
    """The lines ahead of a save: ``first``, the haplotypes, the targets, the samples (``samples`` None: not these) and the command's own."""
    LOG.info(first)
    LOG.info("Number of haplotypes: {:,}".format(m.num_haplotypes))
    LOG.info("Number of reference targets: {:,}".format(m.num_loci))
    if samples is not None:
        LOG.info(samples.format(m.num_samples))
    for line in rest:
        LOG.info(line)


def sample_column(m, sample, ec_filename):
    """The column of the sample named ``sample`` (None stays None: all of them); a name the ``.bin`` does not hold is a KeyError."""
    if sample is None:
        return None
    if sample not in m.sname:
        raise KeyError("sample {} is not in {}".format(sample, ec_filename))
    return m.sname.index(sample)


def check_model(model, groups):
    """What ``ecquant`` and ``ecquant-cells`` refuse before they read anything: a model other than 1..4, or 1..3 without a group file."""
    if model not in (1, 2, 3, 4):
        raise ValueError("model {} is not one of 1, 2, 3, 4".format(model))
    if model != 4 and groups is None:
        raise ValueError("model {} needs a group file (-g/--groups)".format(model))


def ecload(ec_filename):
    """Read EC format 2 -> :class:`ECMatrices` (``bin_utils.py:32-102``)."""
    with open(ec_filename, 'rb') as f:
        b = f.read()
    o = [0]

    def i32(n=1):
        v = np.frombuffer(b, dtype='<i4', count=n, offset=o[0])
        o[0] += 4 * n
        return v

    def name():
        n = int(i32()[0])
        s = unpack_from('<{}s'.format(n), b, o[0])[0].decode('utf-8')
        o[0] += n
        return s

    fmt = int(i32()[0])
    if fmt == 1:
        raise NotImplementedError
    if fmt != 2:
        raise TypeError('Format 0 is not supported anymore.')
    H = int(i32()[0])
    hname = [name() for _ in range(H)]
    T = int(i32()[0])
    lname, lengths = [], np.zeros((T, H), dtype=float)
    for t in range(T):
        lname.append(name())
        lengths[t] = i32(H)
    S = int(i32()[0])
    sname = [name() for _ in range(S)]
    na, nnz = int(i32()[0]), int(i32()[0])
    A = (i32(na).copy(), i32(nnz).copy(), i32(nnz).copy())
    nn, nnzn = int(i32()[0]), int(i32()[0])
    N = (i32(nn).copy(), i32(nnzn).copy(), i32(nnzn).copy())
    return ECMatrices(hname, lname, lengths, sname, A[0], A[1], A[2], N[0], N[1], N[2])


def ec2emase(ec_file, emase_file, **converters):
    """``.bin`` -> EMASE ``.h5`` (``bin_utils.py:979-995``); the CSR -> per-haplotype CSC conversion runs on the GPU
    (``emase_h5.device_hapcsc``; tests may pass ``hapcsc=`` their checker)."""
    from . import emase_h5
    emase_h5.save(emase_file, ecload(ec_file), title='Converted from {}'.format(ec_file), incidence_only=False, **converters)


def emase2ec(emase_file, ec_file, **converters):
    """EMASE ``.h5`` -> ``.bin`` (``bin_utils.py:998-1028``); ``A = sum_h 2^h M_h`` is built on the GPU
    (``emase_h5.device_csr``; tests may pass ``csr=`` their checker)."""
    from . import emase_h5
    ecsave2(ec_file, emase_h5.load(emase_file, **converters))


def load_groups(m, grp_filename):
    """Group file -> (group names, per group the list of locus ids) -- ``AlignmentPropertyMatrix.load_groups``
    (``AlignmentPropertyMatrix.py:176-191``): every line is ``rstrip().split("\\t")`` into ``gene, tx1, tx2, ...``, no line is
    skipped, and a transcript that is not a target of the ``.bin`` is a KeyError."""
    lid = dict(zip(m.lname, range(m.num_loci)))                       # (a duplicated target name: the last one counts, as dict(zip()))
    gname, groups = [], []
    with open(grp_filename) as fh:
        for curline in fh:
            item = curline.rstrip().split("\t")
            gname.append(item[0])
            groups.append([lid[t] for t in item[1:]])
    return gname, groups


def group_map(m, grp_filename):
    """Group file -> ``(gname, map_ptr, map_idx, lengths)``: what ``ecbundle`` hands to ``ecb.bundle``.  The file is read by
    ``load_groups`` (every line ``gene, tx1, tx2, ...``; a transcript that is not a target is a KeyError); group ``g`` is line ``g``.
    ``map_ptr`` (T + 1) / ``map_idx``: per target the ids of its groups, ascending -- a transcript may be in several groups, or in none; one
    listed twice on a line counts once.  ``lengths[g, h]`` is the largest length of ``g``'s members for haplotype ``h``, 0 for a group
    without members.  A group name on two lines is a ValueError naming it (the reference would write two targets of one name)."""
    gname, groups = load_groups(m, grp_filename)
    seen = set()
    for g in gname:
        if g in seen:
            raise ValueError("{}: group {} is listed more than once".format(grp_filename, g))
        seen.add(g)
    T, H, G = m.num_loci, m.num_haplotypes, len(gname)
    gid = np.repeat(np.arange(G, dtype=np.int64), [len(t) for t in groups])
    tid = np.array([t for tids in groups for t in tids], dtype=np.int64)
    pair = np.unique(tid * max(G, 1) + gid)                            # (target, group) pairs, once each, by target then group
    tid, gid = pair // max(G, 1), pair % max(G, 1)
    map_ptr = np.searchsorted(tid, np.arange(T + 1)).astype(np.int32)
    lens = np.asarray(m.lengths).astype(np.int64).reshape(T, H)
    lengths = np.zeros((G, H), dtype=np.int64)
    np.maximum.at(lengths, gid, lens[tid])
    return gname, map_ptr, gid.astype(np.int32), lengths


def ecbundle(ec_filename, grp_filename, out_filename, device=0):
    """``alntools ecbundle``: the targets of a ``.bin`` collapsed into the groups of a group file (isoforms into genes) -- the
    reference's ``AlignmentPropertyMatrix.bundle(reset=True)`` (``AlignmentPropertyMatrix.py:219-275``), then the rows that have become
    equal folded into one EC as ``ecmerge`` folds them.  The group file is parsed here (``group_map``) before libecb is loaded; A and
    N are bundled on the GPU (``ecb.bundle``): the mask at (row, group) is the OR of the row's masks over the group's transcripts, rows
    with equal (group, mask) sets are one EC, numbered by first appearance, counts add per (EC, sample).  The output's targets are the
    groups in file order, each as long as its longest member; haplotypes and samples are copied.  Any failure is logged as
    ``Error: ...``, no file is written and the exception is raised again (the command line exits with status 1)."""
    with command(KEY, created=out_filename):
        LOG.info("Loading {}...".format(ec_filename))
        m = ecload(ec_filename)
        gname, map_ptr, map_idx, lengths = group_map(m, grp_filename)
        if not gname:
            raise ValueError("{}: no groups".format(grp_filename))
        LOG.info("Bundling {:,} targets into {:,} groups...".format(m.num_loci, len(gname)))
        from . import ecb
        A_N = ecb.bundle(m.indptrA, m.indicesA, m.dataA, m.indptrN, m.indicesN, m.dataN, m.num_loci, m.num_haplotypes, len(gname),
                         map_ptr, map_idx, device=device)
        out = ECMatrices(m.hname, gname, lengths, m.sname, *A_N)
        log_saving("Saving to {}...".format(out_filename), out,
                   "Number of equivalence classes: {:,} (from {:,} rows)".format(out.num_reads, m.num_reads))
        write_bin(out_filename, out)
        LOG.info("Saving completed")


def named_samples(m, samples=None, samples_file=None):
    """What ``ecselect``'s ``-s`` and ``--samples FILE`` name -> a bool array over the ``.bin``'s samples, or None when neither is given
    (all are named).  The file holds one name per line, blank lines ignored; a name twice counts once; a name that is not in the ``.bin``
    is a KeyError naming it."""
    if samples is None and samples_file is None:
        return None
    names = list(samples or [])
    if samples_file is not None:
        with open(samples_file) as fh:
            names += [ln.strip() for ln in fh if ln.strip()]
    sid = dict(zip(m.sname, range(m.num_samples)))
    keep = np.zeros(m.num_samples, dtype=bool)
    for n in names:
        if n not in sid:
            raise KeyError("sample {} is not in the EC file".format(n))
        keep[sid[n]] = True
    return keep


def ecselect(ec_filename, out_filename, row_class=None, samples=None, samples_file=None, mincount=None, device=0):
    """``alntools ecselect``: a part of a ``.bin`` -- the reads of one class (``row_class``: None, ``"unique"``, ``"locus-unique"`` or
    ``"multi"``: the selection of the reference's ``get_unique_reads``, ``AlignmentPropertyMatrix.py:386-427``) in the named samples that
    still count ``max(mincount, 1)`` of them (the cell threshold of the reference's ``bam2ec --multisample``,
    ``bam_utils_multisample.py:596-636``; None: no sample is dropped for its total).  The names are resolved here (``named_samples``)
    before libecb is loaded; A and N are selected on the GPU (``ecb.select``).  Rows that keep no count leave the file, the others keep
    their order; targets, lengths and haplotypes are copied, the samples are the kept ones in the input's order.  A result without a
    sample or without a read is refused.  Any failure is logged as ``Error: ...``, no file is written and the exception is raised again
    (the command line exits with status 1)."""
    with command(KEY, created=out_filename):
        LOG.info("Loading {}...".format(ec_filename))
        m = ecload(ec_filename)
        named = named_samples(m, samples, samples_file)
        from . import ecb
        if row_class not in ecb.ROW_CLASSES:
            raise ValueError("no such read class: {}".format(row_class))
        LOG.info("Selecting {} reads of {:,} samples...".format(row_class or "all", m.num_samples if named is None else int(named.sum())))
        A_N, kept = ecb.select(m.indptrA, m.indicesA, m.dataA, m.indptrN, m.indicesN, m.dataN, m.num_loci, m.num_haplotypes,
                               row_class=row_class, sample_keep=named, min_count=mincount, device=device)
        out = ECMatrices(m.hname, m.lname, m.lengths, [s for s, k in zip(m.sname, kept) if k], *A_N)
        if out.num_samples == 0:
            raise ValueError("no sample left")
        if out.num_reads == 0:
            raise ValueError("no read left")
        log_saving("Saving to {}...".format(out_filename), out, "Number of samples: {:,} (from {:,})".format(out.num_samples, m.num_samples),
                   "Number of ECs: {:,} (from {:,} rows)".format(out.num_reads, m.num_reads), samples=None)
        write_bin(out_filename, out)
        LOG.info("Saving completed")


def downsample_rule(reads=None, fraction=None, equalize=False):
    """What ``ecdownsample`` refuses before it opens a file: anything but exactly one of ``-n/--reads N`` (N >= 1), ``-f/--fraction P``
    (0 < P <= 1) and ``--equalize``.  -> ``"reads"``, ``"fraction"`` or ``"equalize"``."""
    given = [name for name, on in (("-n/--reads", reads is not None), ("-f/--fraction", fraction is not None), ("--equalize", bool(equalize))) if on]
    if len(given) != 1:
        raise ValueError("exactly one of -n/--reads, -f/--fraction and --equalize must be given ({})".format(" and ".join(given) if given else "none is"))
    if reads is not None and int(reads) < 1:
        raise ValueError("-n/--reads {}: the number of reads is at least 1".format(reads))
    if fraction is not None and not 0.0 < float(fraction) <= 1.0:
        raise ValueError("-f/--fraction {}: the fraction is above 0 and at most 1".format(fraction))
    return "reads" if reads is not None else "fraction" if fraction is not None else "equalize"


def downsample_targets(totals, stay, reads=None, fraction=None, equalize=False):
    """``ecdownsample``'s target per column of the input: for a sample that stays ``reads``, ``floor(fraction * M_s)`` taken in float64, or
    the smallest ``M_s`` among the samples that stay; -1 for every other column."""
    rule = downsample_rule(reads, fraction, equalize)
    totals, stay = np.asarray(totals, dtype=np.int64), np.asarray(stay, dtype=bool)
    target = np.full(len(totals), -1, dtype=np.int64)
    if not stay.any():
        return target
    if rule == "reads":
        target[stay] = int(reads)
    elif rule == "fraction":
        target[stay] = np.floor(np.float64(fraction) * totals[stay].astype(np.float64)).astype(np.int64)
    else:
        target[stay] = totals[stay].min()
    return target


def ecdownsample(ec_filename, out_filename, reads=None, fraction=None, equalize=False, seed=0, samples=None, samples_file=None, mincount=None,
                 stats_file=None, device=0):
    """``alntools ecdownsample``: the samples of a ``.bin`` thinned to a read depth -- ``reads`` of every sample's reads, or the
    ``fraction`` of them, or (``equalize``) as many as the shallowest sample has, drawn WITHOUT replacement on the GPU
    (``ecb_downsample``: the rule is ``include/ecb_downsample.h``'s).  The steps, in this order: the totals ``M_s``; the samples that stay
    are the named ones (``named_samples``; none named: all) with ``M_s >= max(mincount, 1)``; the target per column of the INPUT
    (:func:`downsample_targets`); the draw on the input's N, so that a sample's result depends on its own column number and on no other
    sample; ``ecb.select`` with every read class, the samples that stay and a threshold of 1 -- the zero entries go, then the rows
    without a read, then the samples thinned to nothing.  Targets, lengths and haplotypes are copied.  ``stats_file``: a tab-separated
    table ``sample, reads_in, reads_out, ecs_in, ecs_out`` under a header line, one line per sample that stays.  A result without a sample
    or without a read is refused.  Any failure is logged as ``Error: ...``, no file is written and the exception is raised again (the
    command line exits with status 1)."""
    opened = []
    with command(KEY, created=out_filename, written=opened):
        downsample_rule(reads, fraction, equalize)
        LOG.info("Loading {}...".format(ec_filename))
        m = ecload(ec_filename)
        named = named_samples(m, samples, samples_file)
        ptr, data = np.asarray(m.indptrN, dtype=np.int64), np.asarray(m.dataN, dtype=np.int64)
        cum = np.concatenate([[0], np.cumsum(data)])
        totals = cum[ptr[1:]] - cum[ptr[:-1]]
        stay = (totals >= max(int(mincount or 0), 1)) & (np.ones(m.num_samples, dtype=bool) if named is None else named)
        target = downsample_targets(totals, stay, reads, fraction, equalize)
        LOG.info("Downsampling {:,} of {:,} samples...".format(int(stay.sum()), m.num_samples))
        from . import ecb, ecb_downsample
        thin, reads_in, reads_out = ecb_downsample.downsample(m.indptrN, m.indicesN, m.dataN, m.num_reads, target, seed=seed, device=device)
        A_N, kept = ecb.select(m.indptrA, m.indicesA, m.dataA, m.indptrN, m.indicesN, thin, m.num_loci, m.num_haplotypes,
                               row_class=None, sample_keep=stay, min_count=1, device=device)
        out = ECMatrices(m.hname, m.lname, m.lengths, [s for s, k in zip(m.sname, kept) if k], *A_N)
        if out.num_samples == 0:
            raise ValueError("no sample left")
        if out.num_reads == 0:
            raise ValueError("no read left")
        if stats_file:
            nz = lambda d: np.diff(np.concatenate([[0], np.cumsum(np.asarray(d) > 0)])[ptr])      # noqa: E731
            ecs_in, ecs_out = nz(m.dataN), nz(thin)
            opened.append(stats_file)
            with open(stats_file, "w") as fh:
                fh.write("sample\treads_in\treads_out\tecs_in\tecs_out\n")
                for s in np.flatnonzero(stay):
                    fh.write("{}\t{}\t{}\t{}\t{}\n".format(m.sname[s], int(reads_in[s]), int(reads_out[s]), int(ecs_in[s]), int(ecs_out[s])))
        log_saving("Saving to {}...".format(out_filename), out, "Number of samples: {:,} (from {:,})".format(out.num_samples, m.num_samples),
                   "Number of ECs: {:,} (from {:,} rows)".format(out.num_reads, m.num_reads),
                   "Number of reads: {:,} (from {:,})".format(int(np.asarray(reads_out)[stay].sum()), int(totals.sum())), samples=None)
        write_bin(out_filename, out)
        LOG.info("Saving completed")


def genotype_mask(m, gt_filename, gname, groups):
    """Genotype file -> ``mask u32[T]`` (bit h = haplotype h allowed at that locus) -- ``AlignmentPropertyMatrix.apply_genotypes``
    (``AlignmentPropertyMatrix.py:483-505``): the leading lines that start with ``#`` are skipped; every later line gives ``gene,
    genotype = item[:2]``; each character of the genotype is a haplotype name (looked up first), the gene is a group name (the last
    group line of that name counts); every transcript of the gene gets the genotype's haplotypes.  Transcripts of no listed gene get 0."""
    from itertools import dropwhile
    hid = dict(zip(m.hname, range(m.num_haplotypes)))
    gid = dict(zip(gname, range(len(gname))))
    mask = np.zeros(m.num_loci, dtype=np.uint32)
    with open(gt_filename) as fh:
        for curline in dropwhile(lambda s: s.startswith('#'), fh):
            item = curline.rstrip().split("\t")
            g, gt = item[:2]
            hids = [hid[c] for c in gt]
            tids = groups[gid[g]]
            if not hids or not tids:                                  # (np.meshgrid of an empty float array indexes gtmask)
                raise IndexError("arrays used as indices must be of integer (or boolean) type")
            bits = 0
            for h in hids:
                bits |= 1 << h
            mask[np.asarray(tids, dtype=np.int64)] |= np.uint32(bits)
    return mask


def apply_genotypes(ec_filename, gt_filename, grp_filename, out_filename, device=0):
    """``alntools apply-genotypes`` (``bin_utils.py:1031-1051``): the ``.bin``'s alignments that the genotypes do not allow are
    removed -- the mask is parsed here, applied to CSR A on the GPU (``ecb.apply_mask``); rows that lose every alignment stay, as
    empty rows.  N: a multisample file's is written back as it was read; a single sample's goes through the reference's dense count
    vector (``ecload`` / ``ecsave2``: duplicates added, zero counts dropped).  Any failure is logged as ``Error: ...`` and no file is
    written, as in the reference (which returns normally then)."""
    from . import ecb
    with command(SWALLOW, created=out_filename):
        LOG.info("Loading {}...".format(ec_filename))
        m = ecload(ec_filename)
        gname, groups = load_groups(m, grp_filename)
        LOG.info("Applying genotypes to the alignment profile...")
        mask = genotype_mask(m, gt_filename, gname, groups)
        m.indptrA, m.indicesA, m.dataA = ecb.apply_mask(m.indptrA, m.indicesA, m.dataA, mask, m.num_haplotypes, device=device)
        converted = False
        if m.num_samples == 1:
            E = m.num_reads
            lo, hi = int(m.indptrN[0]), int(m.indptrN[1])
            count = np.bincount(m.indicesN[lo:hi], weights=m.dataN[lo:hi], minlength=E)
            rows = np.flatnonzero(count)
            m.indptrN = np.array([0, len(rows)], dtype=np.int32)
            m.indicesN, m.dataN = rows.astype(np.int32), count[rows].astype(int).astype(np.int32)
            converted = True
        log_saving("Saviing to {}...".format(out_filename), m,          # (sic: the reference's line)
                   "Saving alignment incidence matrix...", "Saving EC count matrix...", *(['N matrix converted to csc_matrix.'] if converted else []))
        ecsave2(out_filename, m)
        LOG.info("Saving completed")


def counts_table(lname, hname, aln, uniq, locus_uniq):
    """The text of the reference's ``report_alignment_counts`` (``AlignmentPropertyMatrix.py:450-462``): a header ``locus, aln_<h>...,
    uniq_<h>..., locus_uniq`` and one tab-separated line per target, every number as the reference's float64 sums print (``12.0``)."""
    cnt = np.vstack((np.asarray(aln), np.asarray(uniq), np.asarray(locus_uniq)[None, :]))
    out = ["locus\t" + "\t".join('aln_%s' % h for h in hname) + "\t" + "\t".join('uniq_%s' % h for h in hname) + "\t" + "locus_uniq" + "\n"]
    for t, name in enumerate(lname):
        out.append("\t".join([name] + [str(float(v)) for v in cnt[:, t]]) + "\n")
    return "".join(out)


def count_alignments(ec_filename, out_filename, sample=None, device=0):
    """``alntools count-alignments`` (EMASE's command of that name; ``AlignmentPropertyMatrix.report_alignment_counts``): the ``.bin``'s
    alignment counts, allele-unique counts and locus-unique counts per target, counted on the GPU (``ecb.count_alignments``) and written
    as the reference's table.  A multisample file, on which the reference raises, is counted over all its samples, or over the one
    named ``sample``.  A failure is logged as ``Error: ...`` and raised again."""
    from . import ecb
    with command(KEY, created=out_filename):
        LOG.info("Loading {}...".format(ec_filename))
        m = ecload(ec_filename)
        col = sample_column(m, sample, ec_filename)
        LOG.info("Counting alignments...")
        aln, uniq, locus_uniq = ecb.count_alignments(m.indptrA, m.indicesA, m.dataA, m.num_loci, m.num_haplotypes, m.indptrN, m.indicesN,
                                                     m.dataN, sample=col, device=device)
        with open(out_filename, 'w') as fh:
            fh.write(counts_table(m.lname, m.hname, aln, uniq, locus_uniq))


def quant_table(lname, hname, theta):
    """The text ``ecquant`` writes: a header ``locus, <haplotype names>, total`` and one tab-separated line per target, every number as
    :func:`counts_table` writes them (``str(float(v))``, which reads back to the same float64)."""
    theta = np.asarray(theta, dtype=np.float64)
    out = ["locus\t" + "\t".join(hname) + "\ttotal\n"]
    for t, name in enumerate(lname):
        out.append("\t".join([name] + [str(float(v)) for v in theta[:, t]] + [str(float(theta[:, t].sum()))]) + "\n")
    return "".join(out)


def length_scale(m, aln):
    """``ecquant -l``: ``scale[h, t] = 1 / length[t, h]``.  A (target, haplotype) with alignments (``aln[h, t] > 0``) and a length <= 0 is a
    ValueError naming it; any other with a length <= 0 gets scale 0."""
    lens = np.asarray(m.lengths, dtype=np.float64)[:, :m.num_haplotypes].T
    bad = np.argwhere((lens <= 0) & (np.asarray(aln) > 0))
    if len(bad):
        h, t = bad[0]
        raise ValueError("target {} haplotype {} has alignments and length {:g}: cannot scale by its length".format(m.lname[t], m.hname[h], lens[h, t]))
    scale = np.zeros_like(lens)
    np.divide(1.0, lens, out=scale, where=lens > 0)
    return scale


def gene_ids(m, grp_filename):
    """Group file -> ``(gene, names)``: ``gene[t]`` (int32, T) is the gene of target ``t``, what ``ecquant -M 1..3`` hands to
    ``ecb.quantify_model``, and ``names`` the genes' names.  The file is read by :func:`load_groups` (a transcript that is not a target is a
    KeyError).  Genes are numbered in file order, a line with no members adds none; a target on no line is a gene of its own, named after
    itself and numbered after the file's genes in target order.  A target in two groups, or a group name on two lines, is a ValueError
    naming it (one listed twice on a line counts once)."""
    gname, groups = load_groups(m, grp_filename)
    gene = np.full(m.num_loci, -1, dtype=np.int32)
    names, seen = [], set()
    for g, tids in zip(gname, groups):
        if g in seen:
            raise ValueError("{}: group {} is listed more than once".format(grp_filename, g))
        seen.add(g)
        if not tids:
            continue
        for t in tids:
            if gene[t] not in (-1, len(names)):
                raise ValueError("{}: target {} is in two groups ({} and {})".format(grp_filename, m.lname[t], names[gene[t]], g))
            gene[t] = len(names)
        names.append(g)
    for t in np.flatnonzero(gene < 0):
        gene[t] = len(names)
        names.append(m.lname[t])
    return gene, names


def ecquant(ec_filename, out_filename, sample=None, use_lengths=False, max_iters=1000, tol=1e-6, device=0, model=4, groups=None,
            posterior_file=None, hapcsc=None):
    """``alntools ecquant``: EM abundance estimates of a ``.bin`` (``ecb.quantify``: the reference's ``multiply`` / ``normalize_reads`` /
    ``sum`` iterated on the GPU), written as a table of ``locus, <haplotypes>, total`` in read units.  A multisample file is quantified over
    all its samples pooled, or over the one named ``sample``.  ``use_lengths``: every abundance is weighted by 1 / its target's length
    (:func:`length_scale`).  ``model`` 1, 2 or 3: one of EMASE's hierarchical models over the genes of the group file ``groups``
    (:func:`gene_ids`, ``ecb.quantify_model``); without ``groups`` they are refused by name.  ``model`` 4, the default, is the flat step, and
    ``groups`` then changes nothing.  ``posterior_file``: an EMASE ``.h5`` as ``ec2emase`` writes it whose per-haplotype ``data`` is the
    posterior probability of every alignment at the theta the table holds (``ecb.posterior`` with the run's scale, model and genes, then
    ``ecb_csr_to_hapcsc_values``), zeros stored, so the file's incidence is the ``.bin``'s (``hapcsc``: tests may pass a factory that takes
    the values in bit order and returns the conversion ``emase_h5.save`` is to use).  A failure is logged as ``Error: ...`` and raised again; no file is written then: when
    either file cannot be written, neither is left behind."""
    from . import ecb
    written = []                               # (a file that could not be finished, and the one written before it; never one this run did not open)
    with command(KEY, created=out_filename, written=written):
        check_model(model, groups)
        LOG.info("Loading {}...".format(ec_filename))
        m = ecload(ec_filename)
        col = sample_column(m, sample, ec_filename)
        args = (m.indptrA, m.indicesA, m.dataA, m.num_loci, m.num_haplotypes, m.indptrN, m.indicesN, m.dataN)
        gene = names = None
        if model != 4:
            gene, names = gene_ids(m, groups)
        scale = None
        if use_lengths:
            aln = ecb.count_alignments(*args, sample=col, device=device)[0]       # (theta_0 is this aln: no need for ecquant's own set-up twice)
            scale = length_scale(m, aln)
        if model == 4:
            LOG.info("Estimating abundances...")
            theta, info = ecb.quantify(*args, sample=col, scale=scale, max_iters=max_iters, tol=tol, device=device)
        else:
            LOG.info("Estimating abundances (model {}, {:,} genes)...".format(model, len(names)))
            theta, info = ecb.quantify_model(*args, gene=gene, n_genes=len(names), model=model, sample=col, scale=scale, max_iters=max_iters,
                                             tol=tol, device=device)
        LOG.info("iterations: {:,}; delta: {!r}; explained reads: {:,}; {}".format(info["n_iter"], info["delta"], info["explained"],
                                                                                  "converged" if info["converged"] else "not converged"))
        table = quant_table(m.lname, m.hname, theta)
        if posterior_file is not None:
            from . import emase_h5
            LOG.info("Computing the posterior of every alignment...")
            post = ecb.posterior(m.indptrA, m.indicesA, m.dataA, m.num_loci, m.num_haplotypes, theta, scale=scale, gene=gene,
                                 n_genes=0 if names is None else len(names), model=model, device=device)[0]
            convert = hapcsc(post) if hapcsc is not None else emase_h5.device_hapcsc_values(post, device)
            with open(posterior_file, 'wb'):           # (created or truncated: from here on the file is this run's, and goes if the run fails)
                written.append(posterior_file)
            emase_h5.save(posterior_file, m, title='Posterior from {}'.format(ec_filename), incidence_only=False, hapcsc=convert)
        with open(out_filename, 'w') as fh:
            written.append(out_filename)
            fh.write(table)


def boot_table(lname, hname, theta, mean, sd, tot_mean, tot_sd):
    """The text ``ecboot`` writes: a header ``locus``, then per haplotype ``<h>, <h>_mean, <h>_sd``, then ``total, total_mean, total_sd``, and
    one tab-separated line per target: the point estimate as :func:`quant_table` writes it, the bootstrap's mean and standard deviation beside
    it; every number ``str(float(v))``."""
    theta, mean, sd = (np.asarray(a, dtype=np.float64) for a in (theta, mean, sd))
    tot_mean, tot_sd = np.asarray(tot_mean, dtype=np.float64), np.asarray(tot_sd, dtype=np.float64)
    out = ["locus\t" + "\t".join("{0}\t{0}_mean\t{0}_sd".format(h) for h in hname) + "\ttotal\ttotal_mean\ttotal_sd\n"]
    for t, name in enumerate(lname):
        cells = [name]
        for h in range(len(hname)):
            cells += [str(float(theta[h, t])), str(float(mean[h, t])), str(float(sd[h, t]))]
        out.append("\t".join(cells + [str(float(theta[:, t].sum())), str(float(tot_mean[t])), str(float(tot_sd[t]))]) + "\n")
    return "".join(out)


def ecboot(ec_filename, out_filename, n_boot=None, seed=0, sample=None, use_lengths=False, max_iters=1000, tol=1e-6, device=0, model=4, groups=None,
           replicates_file=None):
    """``alntools ecboot``: bootstrap standard errors for ``ecquant``.  ``n_boot`` replicates of the reads of a ``.bin`` (all samples pooled, or
    the one named ``sample``) are redrawn on the GPU under ``seed`` and each is quantified as ``ecquant`` with the same options would
    (``ecb_boot.quantify_bootstrap``); the table (:func:`boot_table`) holds ``ecquant``'s own point estimate from these options and, beside
    it, the mean and the standard deviation over the replicates.  ``replicates_file``: the replicates' estimates, float64 ``[B, H, T]``, as a
    ``.npy``.  A failure is logged as ``Error: ...`` and raised again; no file is written then."""
    from . import ecb, ecb_boot
    written = []
    with command(KEY, created=out_filename, written=written):
        check_model(model, groups)
        if n_boot is None or int(n_boot) < 1:
            raise ValueError("the number of bootstrap replicates (-b) must be at least 1")
        if int(seed) < 0 or int(seed) >= 1 << 64:
            raise ValueError("the seed must be in [0, 2^64)")
        LOG.info("Loading {}...".format(ec_filename))
        m = ecload(ec_filename)
        col = sample_column(m, sample, ec_filename)
        args = (m.indptrA, m.indicesA, m.dataA, m.num_loci, m.num_haplotypes, m.indptrN, m.indicesN, m.dataN)
        gene, names = gene_ids(m, groups) if model != 4 else (None, ())
        scale = None
        if use_lengths:
            scale = length_scale(m, ecb.count_alignments(*args, sample=col, device=device)[0])
        LOG.info("Estimating abundances...")
        if model == 4:
            theta, info = ecb.quantify(*args, sample=col, scale=scale, max_iters=max_iters, tol=tol, device=device)
        else:
            theta, info = ecb.quantify_model(*args, gene=gene, n_genes=len(names), model=model, sample=col, scale=scale, max_iters=max_iters,
                                             tol=tol, device=device)
        LOG.info("iterations: {:,}; delta: {!r}; explained reads: {:,}; {}".format(info["n_iter"], info["delta"], info["explained"],
                                                                                  "converged" if info["converged"] else "not converged"))
        LOG.info("Bootstrapping ({:,} replicates, seed {})...".format(int(n_boot), int(seed)))
        res = ecb_boot.quantify_bootstrap(*args, n_reps=int(n_boot), seed=int(seed), sample=col, scale=scale, max_iters=max_iters, tol=tol, gene=gene,
                                          n_genes=len(names), model=model, device=device, return_reps=replicates_file is not None)
        mean, sd, tot_mean, tot_sd, binfo = res[:5]
        LOG.info("replicates converged: {:,} of {:,}; most iterations: {:,}".format(int(np.sum(binfo["converged"])), int(n_boot),
                                                                                   int(np.max(binfo["n_iter"]))))
        table = boot_table(m.lname, m.hname, theta, mean, sd, tot_mean, tot_sd)
        if replicates_file is not None:
            with open(replicates_file, 'wb') as fh:
                written.append(replicates_file)
                np.save(fh, np.asarray(res[5], dtype=np.float64))
        with open(out_filename, 'w') as fh:
            written.append(out_filename)
            fh.write(table)


def clusters_file(lname, comp_of_locus, multi_only=False, source="the .bin"):
    """The text ``ecclusters`` writes and the components it holds -> ``(text, written)``: a group file as :func:`load_groups` reads it, one
    line per component in component order -- the name of its lowest-numbered target, then all its targets, that one included, in target
    order, tab-separated.  ``multi_only``: the components of one target are left out.  ``written``: the components on the lines, ascending.
    Two targets of one name among those that head a line are a ValueError naming it (``ecbundle`` would refuse the file)."""
    comp = np.asarray(comp_of_locus, dtype=np.int64)
    order = np.argsort(comp, kind="stable")                             # by component, then by target
    sizes = np.bincount(comp, minlength=0)
    ends = np.cumsum(sizes)
    written = np.flatnonzero(sizes >= (2 if multi_only else 1))
    seen = set()
    out = []
    for c in written:
        members = order[ends[c] - sizes[c]:ends[c]]
        head = lname[members[0]]
        if head in seen:
            raise ValueError("{}: two targets named {} would each head a cluster".format(source, head))
        seen.add(head)
        out.append("\t".join([head] + [lname[t] for t in members]) + "\n")
    return "".join(out), written


def clusters_stats(written, comp_loci, comp_ecs, comp_reads):
    """The text of ``ecclusters --stats``: a header ``cluster, targets, ecs, reads`` and one line of integers per written component -- its
    number, its targets, the ECs that tie them together and the reads of those ECs."""
    out = ["cluster\ttargets\tecs\treads\n"]
    for c in written:
        out.append("{}\t{}\t{}\t{}\n".format(int(c), int(comp_loci[c]), int(comp_ecs[c]), int(comp_reads[c])))
    return "".join(out)


def ecclusters(ec_filename, out_filename, sample=None, min_count=1, stats_file=None, multi_only=False, device=0):
    """``alntools ecclusters``: the targets of a ``.bin`` grouped by the reads they share -- the connected components of its target-EC
    incidence, found on the GPU (``ecb_components.components``) -- written as a group file (:func:`clusters_file`) that ``ecbundle`` and
    ``ecquant -M 1|2|3 -g`` take as it stands.  An EC ties its targets together when it counts ``min_count`` reads or more, over all samples
    pooled or in the one named ``sample``.  ``stats_file``: the table of :func:`clusters_stats`.  ``multi_only``: the clusters of one
    target are left out (``gene_ids`` gives an unlisted target a gene of its own, so both files mean the same to ``-M``; ``ecbundle`` drops
    the alignments of an unlisted target, so only the default file loses nothing there).  A failure is logged as ``Error: ...`` and raised
    again; no file is written then."""
    written = []
    with command(KEY, created=out_filename, written=written):
        if int(min_count) < 0:
            raise ValueError("the minimum count (-m) must be at least 0")
        LOG.info("Loading {}...".format(ec_filename))
        m = ecload(ec_filename)
        col = sample_column(m, sample, ec_filename)
        from . import ecb_components
        LOG.info("Finding the clusters of {:,} targets...".format(m.num_loci))
        of_locus, _of_ec, loci, ecs, reads, sizes = ecb_components.components(
            m.indptrA, m.indicesA, m.dataA, m.num_loci, m.num_haplotypes, m.indptrN, m.indicesN, m.dataN, sample=col, min_count=int(min_count),
            device=device)
        n_comp, n_link, largest, n_multi = sizes
        total = int(np.sum(reads))
        big = int(np.argmax(loci)) if n_comp else 0
        LOG.info("Number of clusters: {:,} ({:,} of two targets or more), from {:,} linking ECs".format(n_comp, n_multi, n_link))
        LOG.info("Largest cluster: {:,} targets ({:.1%} of the targets), {:,} reads ({:.1%} of the linking reads)".format(
            largest, largest / max(m.num_loci, 1), int(reads[big]) if n_comp else 0, (int(reads[big]) / total) if total else 0.0))
        text, ids = clusters_file(m.lname, of_locus, multi_only=multi_only, source=ec_filename)
        if stats_file is not None:
            with open(stats_file, 'w') as fh:
                written.append(stats_file)
                fh.write(clusters_stats(ids, loci, ecs, reads))
        with open(out_filename, 'w') as fh:
            written.append(out_filename)
            fh.write(text)


def cells_table(sname, lname, hname, cell_ptr, slot_locus, theta):
    """The text ``ecquant-cells`` writes: a header ``sample, locus, <haplotype names>, total`` and one tab-separated line per slot -- a target
    in the support of a cell -- in cell order, every number as :func:`quant_table` writes them (``str(float(v))``)."""
    theta = np.asarray(theta, dtype=np.float64)
    out = ["sample\tlocus\t" + "\t".join(hname) + "\ttotal\n"]
    for c, name in enumerate(sname):
        for s in range(int(cell_ptr[c]), int(cell_ptr[c + 1])):
            out.append("\t".join([name, lname[int(slot_locus[s])]] + [str(float(v)) for v in theta[s]] + [str(float(theta[s].sum()))]) + "\n")
    return "".join(out)


def cells_report(sname, info, keep=None):
    """The text of ``ecquant-cells --report``: ``sample, n_iter, delta, explained, converged`` (0 or 1), one line per quantified cell."""
    out = ["sample\tn_iter\tdelta\texplained\tconverged\n"]
    for c, name in enumerate(sname):
        if keep is None or keep[c]:
            out.append("%s\t%d\t%s\t%d\t%d\n" % (name, int(info["n_iter"][c]), str(float(info["delta"][c])), int(info["explained"][c]),
                                                 int(bool(info["converged"][c]))))
    return "".join(out)


def ecquant_cells(ec_filename, out_filename, samples=None, samples_file=None, use_lengths=False, max_iters=1000, tol=1e-6, report=None, device=0,
                  model=4, groups=None):
    """``alntools ecquant-cells``: one EM abundance estimate per sample (cell) of a multisample ``.bin`` (``ecb.quantify_cells``: every cell
    over its own support, all iterated together on the GPU), written as :func:`cells_table`; ``report``: a second file, :func:`cells_report`.
    ``samples`` / ``samples_file`` name the cells as for ``ecselect`` (:func:`named_samples`; default: all).  ``use_lengths``: every abundance
    is weighted by 1 / its target's length (:func:`length_scale` on the alignment counts of all samples pooled: what ``ecquant -l`` refuses is
    refused here by the same name).  ``model`` 1, 2 or 3: one of EMASE's hierarchical models over the genes of the group file ``groups``, run
    per cell (:func:`gene_ids`, ``ecb.quantify_cells_model``: the sums over a gene run over the cell's own targets); without ``groups`` they
    are refused by name.  ``model`` 4, the default, is the flat step, and ``groups`` then changes nothing.  A failure is logged as
    ``Error: ...`` and raised again; no file is written then."""
    with command(KEY, created=out_filename):
        check_model(model, groups)
        LOG.info("Loading {}...".format(ec_filename))
        m = ecload(ec_filename)
        keep = named_samples(m, samples, samples_file)
        from . import ecb
        args = (m.indptrA, m.indicesA, m.dataA, m.num_loci, m.num_haplotypes, m.indptrN, m.indicesN, m.dataN)
        scale = None
        if use_lengths:
            scale = length_scale(m, ecb.count_alignments(*args, device=device)[0])
        n_cells = m.num_samples if keep is None else int(keep.sum())
        if model == 4:
            LOG.info("Estimating abundances of {:,} cells...".format(n_cells))
            cell_ptr, slot_locus, theta, info = ecb.quantify_cells(*args, cell_keep=keep, scale=scale, max_iters=max_iters, tol=tol, device=device)
        else:
            gene, names = gene_ids(m, groups)
            LOG.info("Estimating abundances of {:,} cells (model {}, {:,} genes)...".format(n_cells, model, len(names)))
            cell_ptr, slot_locus, theta, info = ecb.quantify_cells_model(*args, gene=gene, n_genes=len(names), model=model, cell_keep=keep, scale=scale,
                                                                         max_iters=max_iters, tol=tol, device=device)
        ran = np.ones(m.num_samples, dtype=bool) if keep is None else keep
        LOG.info("slots: {:,}; most iterations: {:,}; explained reads: {:,}; cells not converged: {:,}".format(
            len(slot_locus), int(np.max(info["n_iter"], initial=0)), int(np.sum(info["explained"])), int(np.sum(~np.asarray(info["converged"])[ran]))))
        table = cells_table(m.sname, m.lname, m.hname, cell_ptr, slot_locus, theta)
        rep = cells_report(m.sname, info, keep) if report is not None else None
        with open(out_filename, 'w') as fh:
            fh.write(table)
        if rep is not None:
            with open(report, 'w') as fh:
                fh.write(rep)


def ecdump(ec_filename):
    """``alntools ecdump`` (``bin_utils.py:959-976``): the shapes of a ``.bin``, as the reference's log lines.  Host only."""
    with command(SWALLOW):
        LOG.info("Loading {}...".format(ec_filename))
        m = ecload(ec_filename)
        LOG.info("Number of reference transcripts (or targets): {:,}".format(m.num_loci))
        LOG.info("Number of haplotypes: {:,}".format(m.num_haplotypes))
        LOG.info("Number of samples: {:,}".format(m.num_samples))
        LOG.info("Number of ECs (or reads): {:,}".format(m.num_reads))
        LOG.info("Shape of alignment incidence matrix: {:,} x {:,} x {:,}".format(*m.shape))
        if m.num_samples > 1:
            LOG.info("Shape of EC count matrix: {:,} x {:,}".format(m.num_reads, m.num_samples))
        elif m.num_samples == 1:
            LOG.info("Shape of EC count matrix: {:,} x {:,}".format(m.num_reads, 1))
        else:
            LOG.error("Error: Something is wrong with EC count matrix")


class MergePlan(object):
    """What ``plan_merge`` decides from the headers alone: the output's names and lengths and, per input, the maps of its
    columns and samples into the output's (``target_maps[k]`` is None when every input has the same target list)."""

    def __init__(self, hname, lname, lengths, sname, target_maps, sample_maps):
        self.hname, self.lname, self.lengths, self.sname = hname, lname, lengths, sname
        self.target_maps, self.sample_maps = target_maps, sample_maps


def plan_merge(ms, names=None):
    """The header side of ``ecmerge``: every input must have the same haplotypes in the same order.  Targets: one identical list
    everywhere is used as it is; otherwise the output's targets are the union by name in first-seen order, and a list that repeats a
    name is then an error.  A name seen in several inputs must have the same per-haplotype lengths.  Samples: the union by name in
    first-seen order; a list that repeats a name is an error.  Raises ValueError with the reason."""
    names = names or ["input {}".format(k + 1) for k in range(len(ms))]
    if not ms:
        raise ValueError("no input files")
    m0 = ms[0]
    for m, f in zip(ms[1:], names[1:]):
        if m.hname != m0.hname:
            raise ValueError("{}: haplotypes {} differ from {}'s {}".format(f, m.hname, names[0], m0.hname))
    H = m0.num_haplotypes
    lens = [np.asarray(m.lengths).astype(np.int64).reshape(m.num_loci, H) for m in ms]
    if all(m.lname == m0.lname for m in ms[1:]):
        for m, L, f in zip(ms[1:], lens[1:], names[1:]):
            bad = np.flatnonzero((L != lens[0]).any(axis=1))
            if len(bad):
                raise ValueError("{}: target {} has lengths {} against {} in {}".format(
                    f, m.lname[bad[0]], L[bad[0]].tolist(), lens[0][bad[0]].tolist(), names[0]))
        lname, lengths, tmaps = list(m0.lname), lens[0], [None] * len(ms)
    else:
        tid, lname, rows, tmaps = {}, [], [], []
        for m, L, f in zip(ms, lens, names):
            if len(set(m.lname)) != len(m.lname):
                dup = next(t for i, t in enumerate(m.lname) if t in m.lname[:i])
                raise ValueError("{}: target {} is listed more than once (the target lists differ, so columns are matched by name)".format(f, dup))
            tm = np.empty(m.num_loci, dtype=np.int64)
            for i, t in enumerate(m.lname):
                j = tid.get(t)
                if j is None:
                    j = tid[t] = len(lname)
                    lname.append(t)
                    rows.append(L[i])
                elif not np.array_equal(rows[j], L[i]):
                    raise ValueError("{}: target {} has lengths {} against {} before".format(f, t, L[i].tolist(), rows[j].tolist()))
                tm[i] = j
            tmaps.append(tm)
        lengths = np.array(rows, dtype=np.int64).reshape(len(lname), H)
    sid, sname, smaps = {}, [], []
    for m, f in zip(ms, names):
        if len(set(m.sname)) != len(m.sname):
            dup = next(s for i, s in enumerate(m.sname) if s in m.sname[:i])
            raise ValueError("{}: sample {} is listed more than once".format(f, dup))
        sm = np.empty(m.num_samples, dtype=np.int64)
        for i, s in enumerate(m.sname):
            if s not in sid:
                sid[s] = len(sname)
                sname.append(s)
            sm[i] = sid[s]
        smaps.append(sm)
    return MergePlan(list(m0.hname), lname, lengths, sname, tmaps, smaps)


def ecmerge(ec_files, ec_out, device=0):
    """``alntools ecmerge`` (the reference's ``bin_utils.ecmerge``, ``bin_utils.py:443-956``, which cannot run): several ``.bin``
    files as one.  The headers are read and planned here (``plan_merge``) before libecb is loaded; A and N are combined on the GPU
    (``ecb.combine``): rows with equal (column, haplotype mask) sets are one EC, numbered by first appearance over the files in
    order, counts add per (EC, sample) and zero sums are dropped.  Any failure is logged as ``Error: ...``, no file is written and
    the exception is raised again (the command line exits with status 1)."""
    with command(RAISE, created=ec_out):
        ms = []
        for f in ec_files:
            LOG.info("Loading {}...".format(f))
            ms.append(ecload(f))
        plan = plan_merge(ms, list(ec_files))
        LOG.info("Combining {:,} files...".format(len(ms)))
        from . import ecb
        parts = [dict(indptrA=m.indptrA, indicesA=m.indicesA, dataA=m.dataA, indptrN=m.indptrN, indicesN=m.indicesN, dataN=m.dataN,
                      n_loci=m.num_loci, target_map=tm, sample_map=sm)
                 for m, tm, sm in zip(ms, plan.target_maps, plan.sample_maps)]
        A_N = ecb.combine(parts, len(plan.lname), len(plan.hname), len(plan.sname), device=device)
        out = ECMatrices(plan.hname, plan.lname, plan.lengths, plan.sname, *A_N)
        log_saving("Saving to {}...".format(ec_out), out,
                   "Number of equivalence classes: {:,} (from {:,} rows)".format(out.num_reads, sum(m.num_reads for m in ms)))
        write_bin(ec_out, out)
        LOG.info("Saving completed")
