"""The UMI rule of ``include/ecb_umi.h`` as a plain loop over reads -- a dict by key and set intersections: what ``ecb_collapse_umis``
must give, byte for byte.  ``tests/test_collapse_umis.py`` holds it to a hand-written dozen of records."""
import numpy as np

UMI_NONE = 0xFFFFFFFFFFFFFFFF
HAP_SHIFT = 16


def passes(hf):
    """``rec_valid`` of ``csrc/ecb.hip`` (``tuples.record_valid`` with the two host bits 12 and 13)."""
    if hf & 0x4:
        return False
    if hf & 0x1:
        if (hf & 0x80) or not (hf & 0x2) or (hf & 0x1000) or (hf & 0x2000):
            return False
    return True


def reads_of(read_id, hapflag):
    """The reads of a sound stream: a list of lists of record indices, every record of the read, passing or not.  The records in
    front that carry the id before the first read's belong to no read."""
    reads, prev = [], None
    for i in range(len(read_id)):
        r = int(read_id[i])
        if reads and r == prev:
            reads[-1].append(i)
        elif passes(int(hapflag[i])):            # the first passing record, or a step (which the contract puts on a passing record)
            reads.append([i])
            prev = r
        elif reads:
            raise AssertionError("record %d: not a sound stream" % i)
        elif prev is None:
            prev = r
        elif r != prev:
            raise AssertionError("record %d: not a sound stream" % i)
    return reads


def breach(read_id, locus, hapflag, n_reads, n_loci, n_haps):
    """``(record, reason)`` of the lowest record that breaks the contract, or None.  The count of reads is looked at last, on a stream
    that is otherwise sound."""
    for i in range(len(read_id)):
        hf = int(hapflag[i])
        d = (int(read_id[i]) - int(read_id[i - 1])) % (1 << 32) if i else 0
        if d == 1:
            if not passes(hf):
                return i, "read_id steps on a record that does not pass the filter"
        elif d != 0:
            return i, "read_id steps by more than 1" if d < (1 << 31) else "read_id falls"
        if passes(hf):
            if int(locus[i]) >= n_loci:
                return i, "locus at or beyond n_loci"
            if hf >> HAP_SHIFT >= n_haps:
                return i, "haplotype at or beyond n_haps"
    reads = reads_of(read_id, hapflag)
    if len(reads) != n_reads:
        at = reads[n_reads][0] if len(reads) > n_reads else len(read_id) - 1
        return at, "the stream holds %d reads, n_reads is %d" % (len(reads), n_reads)
    return None


def collapse(read_id, locus, hapflag, mol_key):
    """-> ``(read_id, locus, hapflag, first_read, counts)`` of a sound stream whose read r has the key ``mol_key[r]``."""
    reads = reads_of(read_id, hapflag)
    assert len(reads) == len(mol_key)
    molecules = {}                               # key -> reads, in order; the dict keeps the order of first reads
    n_none = 0
    for r in range(len(reads)):
        k = int(mol_key[r])
        if k == UMI_NONE:
            n_none += 1
            k = ("none", r)
        molecules.setdefault(k, []).append(r)
    out_id, out_loc, out_hf, first = [], [], [], []
    n_multi = n_gone = 0
    for members in molecules.values():           # (every key's first read is lower than the next key's: insertion order)
        if len(members) == 1:
            records = [(int(locus[i]), int(hapflag[i])) for i in reads[members[0]] if passes(int(hapflag[i]))]
        else:
            n_multi += 1
            common = None
            for r in members:
                targets = {(int(locus[i]), int(hapflag[i]) >> HAP_SHIFT) for i in reads[r] if passes(int(hapflag[i]))}
                common = targets if common is None else common & targets
            records = [(l, h << HAP_SHIFT) for l, h in sorted(common)]
        if not records:
            n_gone += 1
            continue
        for l, hf in records:
            out_id.append(len(first)); out_loc.append(l); out_hf.append(hf)
        first.append(members[0])
    counts = (len(reads), len(molecules), n_multi, n_gone, len(out_id), n_none)
    u32 = lambda a: np.array(a, dtype=np.uint32)
    return u32(out_id), u32(out_loc), u32(out_hf), u32(first), counts
