# -*- coding: utf-8 -*-
"""Minimal BGZF / BAM reader and writer (zlib only).

The reference decodes BAM through pysam/htslib (``bam_utils.py:253-259``); that
stays on the host in this build too.  pysam is used when it is importable;
otherwise this module supplies the handful of raw BAM fields the hot path
consumes (``flag, refID, pos, next_refID, next_pos, read_name`` -- the fields
behind the pysam attributes read at ``bam_utils.py:264-301``).

The writer exists so that tests and the synthetic-workload generator can make
real ``.bam`` files without samtools.  It writes the 16-byte BGZF block header
and the 28-byte EOF block byte-for-byte as htslib does (the reference checks
both literally, ``bam_utils.py:29-30,134-154``).
"""
from __future__ import annotations

import os
import struct
import zlib

import numpy as np

BGZF_HEADER = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00\x42\x43\x02\x00"
BGZF_EOF = (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00"
            b"\x1b\x00\x03\x00\x00\x00\x00\x00\x00\x00\x00\x00")
_MAX_BLOCK = 0xFF00  # uncompressed payload per BGZF block (htslib's choice)

_REC_FIXED = struct.Struct("<iiiBBHHHiiii")  # block_size .. tlen (36 bytes)


# --------------------------------------------------------------------------- #
# BGZF
# --------------------------------------------------------------------------- #
def bgzf_block(data: bytes, level: int = 6) -> bytes:
    """One complete BGZF block holding ``data`` (<= 64 KiB uncompressed)."""
    if len(data) > 0x10000:
        raise ValueError("BGZF block payload too large")
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    comp = c.compress(data) + c.flush()
    bsize = len(comp) + 25  # header 18 incl. BSIZE field, trailer 8, minus 1
    if bsize > 0xFFFF:
        # incompressible: store
        c = zlib.compressobj(0, zlib.DEFLATED, -15)
        comp = c.compress(data) + c.flush()
        bsize = len(comp) + 25
    return (BGZF_HEADER + struct.pack("<H", bsize) + comp +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


class BgzfWriter(object):
    def __init__(self, path, mode="wb", level=6):
        self._fh = open(path, mode)
        self._buf = bytearray()
        self._level = level

    def write(self, data):
        self._buf += data
        while len(self._buf) >= _MAX_BLOCK:
            self._fh.write(bgzf_block(bytes(self._buf[:_MAX_BLOCK]), self._level))
            del self._buf[:_MAX_BLOCK]

    def flush_block(self):
        """End the current BGZF block here (next write starts a new block)."""
        if self._buf:
            self._fh.write(bgzf_block(bytes(self._buf), self._level))
            self._buf = bytearray()

    def close(self, eof=True):
        self.flush_block()
        if eof:
            self._fh.write(BGZF_EOF)
        self._fh.close()


def iter_bgzf_blocks(fh):
    """Yield ``(file_offset, payload_bytes)`` for every BGZF block of ``fh``."""
    while True:
        start = fh.tell()
        head = fh.read(12)
        if not head:
            return
        if len(head) < 12 or head[:4] != b"\x1f\x8b\x08\x04":
            raise ValueError("not a BGZF block at offset %d" % start)
        xlen = struct.unpack_from("<H", head, 10)[0]
        extra = fh.read(xlen)
        bsize = None
        off = 0
        while off < xlen:
            si = extra[off:off + 2]
            slen = struct.unpack_from("<H", extra, off + 2)[0]
            if si == b"BC":
                bsize = struct.unpack_from("<H", extra, off + 4)[0] + 1
            off += 4 + slen
        if bsize is None:
            raise ValueError("BGZF block without BC subfield at %d" % start)
        comp = fh.read(bsize - 12 - xlen - 8)
        crc, isize = struct.unpack("<II", fh.read(8))
        data = zlib.decompress(comp, -15) if isize else b""
        if len(data) != isize:
            raise ValueError("BGZF block size mismatch at %d" % start)
        yield start, data


# --------------------------------------------------------------------------- #
# BAM writer
# --------------------------------------------------------------------------- #
def _reg2bin(beg, end):
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


_AUX_FMT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}    # the aux types of a fixed size, but 'A'
_AUX_INT = "cCsSiI"


def pack_tags(tags):
    """The aux fields of a record: ``tags`` = ``(tag, type, value)`` triples, ``type`` one of ``A c C s S i I f Z H B``; the value of a
    ``B`` is ``(subtype, values)``."""
    out = bytearray()
    for tag, typ, value in tags:
        if len(tag) != 2:
            raise ValueError("an aux tag is two characters: %r" % (tag,))
        out += tag.encode("ascii") + typ.encode("ascii")
        if typ == "A":
            out += value.encode("ascii")[:1]
        elif typ in _AUX_FMT:
            out += struct.pack(_AUX_FMT[typ], value)
        elif typ in "ZH":
            out += value.encode("ascii") + b"\x00"
        elif typ == "B":
            sub, values = value
            out += sub.encode("ascii") + struct.pack("<i", len(values)) + b"".join(struct.pack(_AUX_FMT[sub], v) for v in values)
        else:
            raise ValueError("unknown aux type %r" % (typ,))
    return bytes(out)


def pack_record(qname, flag, ref_id, pos, next_ref_id=-1, next_pos=-1, mapq=255, tlen=0, tags=None):
    """One BAM alignment record with an empty CIGAR/SEQ/QUAL (allowed by the spec); ``tags``: its aux fields (:func:`pack_tags`)."""
    name = qname.encode("utf-8") + b"\x00"
    if len(name) > 255:
        raise ValueError("read name too long for BAM")
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(name), mapq,
                       _reg2bin(max(pos, 0), max(pos, 0) + 1), 0, flag & 0xFFFF, 0,
                       next_ref_id, next_pos, tlen) + name
    if tags:
        body += pack_tags(tags)
    return struct.pack("<i", len(body)) + body


def record_score(rec, tag_a, tag_b=None):
    """``(score, present)`` of the record ``rec`` -- its bytes behind ``block_size`` -- as ``bd_set_score`` / ``bd_scores`` of
    ``include/bamdec.h`` define them: the aux fields walked behind the name, the CIGAR, the sequence and the qualities, every step
    bounded by the record; ``tag_a``'s integer value, plus ``tag_b``'s where the record has one, clamped to int32; ``present``: the
    record has ``tag_a``.  A field that runs past the record, an unknown type or a score tag that is no integer: ``ValueError``."""
    bs = len(rec)
    l_name, n_cigar = rec[8], rec[12] | (rec[13] << 8)
    (l_seq,) = struct.unpack_from("<i", rec, 16)
    if l_seq < 0:
        raise ValueError("BAM record: negative sequence length")
    off = 32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq
    if off > bs:
        raise ValueError("BAM record: CIGAR, sequence or qualities run past the record")
    past = ValueError("BAM record: an aux field runs past the record")
    ta, tb = tag_a.encode("ascii"), (tag_b.encode("ascii") if tag_b else None)
    a = b = 0
    has_a = False
    while off < bs:
        if off + 3 > bs:
            raise past
        tag, typ = rec[off:off + 2], chr(rec[off + 2])
        off += 3
        if typ == "A" or typ in _AUX_FMT:
            size = 1 if typ == "A" else struct.calcsize(_AUX_FMT[typ])
            if off + size > bs:
                raise past
        elif typ in "ZH":
            z = rec.find(b"\x00", off)
            if z < 0:
                raise past
            size = z - off + 1
        elif typ == "B":
            if off + 5 > bs:
                raise past
            sub = chr(rec[off])
            (count,) = struct.unpack_from("<i", rec, off + 1)
            if sub not in _AUX_FMT or count < 0:
                raise ValueError("BAM record: an aux array of an unknown type or a negative length")
            size = 5 + struct.calcsize(_AUX_FMT[sub]) * count
            if off + size > bs:
                raise past
        else:
            raise ValueError("BAM record: an aux field of an unknown type")
        if tag == ta or (tb is not None and tag == tb):
            if typ not in _AUX_INT:
                raise ValueError("BAM record: the score tag is not an integer")
            (v,) = struct.unpack_from(_AUX_FMT[typ], rec, off)
            if tag == ta:
                a, has_a = v, True
            else:
                b = v
        off += size
    return max(-(1 << 31), min((1 << 31) - 1, a + b)), has_a


def write_bam(path, references, records, header_text=None, level=6, tags=None):
    """Write a BAM file.

    ``references``: sequence of ``(name, length)``; ``records``: iterable of
    ``(qname, flag, ref_id, pos, next_ref_id, next_pos)``.  The header ends on a
    BGZF block boundary, as samtools writes it (the reference's single-chunk path
    relies on that, ``bam_utils.py:87-99,172,184``).  ``tags``: the aux fields of
    every record, one list of ``(tag, type, value)`` per record (:func:`pack_tags`);
    without it the records carry none.
    """
    if header_text is None:
        header_text = "@HD\tVN:1.0\tSO:unsorted\n" + "".join(
            "@SQ\tSN:%s\tLN:%d\n" % (n, l) for n, l in references)
    text = header_text.encode("utf-8")
    w = BgzfWriter(path, level=level)
    hdr = bytearray(b"BAM\x01" + struct.pack("<i", len(text)) + text +
                    struct.pack("<i", len(references)))
    for n, l in references:
        nb = n.encode("utf-8") + b"\x00"
        hdr += struct.pack("<i", len(nb)) + nb + struct.pack("<i", l)
    w.write(bytes(hdr))
    w.flush_block()
    if tags is None:
        for r in records:
            w.write(pack_record(*r))
    else:
        for r, t in zip(records, tags):
            w.write(pack_record(*r, tags=t))
    w.close()


# --------------------------------------------------------------------------- #
# BAM reader
# --------------------------------------------------------------------------- #
class BamReader(object):
    """Sequential BAM reader exposing the raw fields of each record.

    ``references`` / ``lengths`` mirror ``pysam.AlignmentFile.references/.lengths``
    (used at ``bam_utils.py:582,615``).
    """

    def __init__(self, path):
        self.path = path
        self._fh = open(path, "rb")
        self._size = os.path.getsize(path)
        self._blocks = iter_bgzf_blocks(self._fh)
        self._buf = b""
        self._pos = 0
        self._score_tags = None          # set_score: (tag_a, tag_b or None)
        self._scores = []                # (score, present) of the records handed out since read_batch last began
        self._read_header()

    def set_score(self, tag_a, tag_b=None):
        """As ``bd_set_score``: from here on every record's score is worked out (:func:`record_score`), and :meth:`scores` returns
        those of the records the last :meth:`read_batch` handed out.  ``tag_a`` None switches it off."""
        self._score_tags = None if tag_a is None else (tag_a, tag_b)
        self._scores = []

    def scores(self):
        """-> ``(score int32, present uint8)`` of the records of the last :meth:`read_batch`."""
        return (np.array([s for s, _ in self._scores], dtype=np.int32), np.array([p for _, p in self._scores], dtype=np.uint8))

    # -- byte supply ---------------------------------------------------------
    def _need(self, n):
        while len(self._buf) - self._pos < n:
            try:
                _, data = next(self._blocks)
            except StopIteration:
                return False
            self._buf = self._buf[self._pos:] + data
            self._pos = 0
        return True

    def _take(self, n):
        if not self._need(n):
            raise EOFError("truncated BAM")
        b = self._buf[self._pos:self._pos + n]
        self._pos += n
        return b

    def _read_header(self):
        if self._take(4) != b"BAM\x01":
            raise ValueError("%s is not a BAM file" % self.path)
        l_text = struct.unpack("<i", self._take(4))[0]
        self.text = self._take(l_text).decode("utf-8", "replace")
        n_ref = struct.unpack("<i", self._take(4))[0]
        names, lens = [], []
        for _ in range(n_ref):
            l_name = struct.unpack("<i", self._take(4))[0]
            names.append(self._take(l_name)[:-1].decode("utf-8"))
            lens.append(struct.unpack("<i", self._take(4))[0])
        self.references = tuple(names)
        self.lengths = tuple(lens)

    # -- records -------------------------------------------------------------
    def __iter__(self):
        return self

    def __next__(self):
        """-> ``(qname, flag, ref_id, pos, next_ref_id, next_pos)``"""
        if not self._need(4):
            raise StopIteration
        (bs,) = struct.unpack_from("<i", self._buf, self._pos)
        if not self._need(4 + bs):
            raise EOFError("truncated BAM record")
        p = self._pos
        (_, ref_id, pos, l_name, _mq, _bin, _nc, flag, _ls, nref, npos,
         _tl) = _REC_FIXED.unpack_from(self._buf, p)
        qname = self._buf[p + 36:p + 36 + l_name - 1].decode("utf-8")
        if self._score_tags is not None:
            self._scores.append(record_score(self._buf[p + 4:p + 4 + bs], *self._score_tags))
        self._pos = p + 4 + bs
        return qname, flag, ref_id, pos, nref, npos

    def progress(self):
        """Fraction of the file's (compressed) bytes taken in so far."""
        return min(1.0, self._fh.tell() / float(self._size)) if self._size else 0.0

    def read_batch(self, max_records):
        """Up to ``max_records`` records as column arrays
        ``(qnames list, flag u16, ref_id i32, pos i32, next_ref_id i32, next_pos i32)``."""
        q, cols = [], []
        self._scores = []
        for _ in range(max_records):
            try:
                r = self.__next__()
            except StopIteration:
                break
            q.append(r[0])
            cols.append(r[1:])
        a = np.asarray(cols, dtype=np.int64).reshape(-1, 5)
        return (q, a[:, 0].astype(np.uint16), a[:, 1].astype(np.int32), a[:, 2].astype(np.int32),
                a[:, 3].astype(np.int32), a[:, 4].astype(np.int32))

    def close(self):
        self._fh.close()
