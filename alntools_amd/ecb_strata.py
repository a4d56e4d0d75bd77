# -*- coding: utf-8 -*-
"""``--best-strata``'s bindings: ``ecb_best_strata`` / ``ecb_best_strata_device`` of ``libecb.so`` (``include/ecb_strata.h``), bound lazily
on the library :func:`alntools_amd.ecb.load` returns, with a symbol tuple and a signature table of their own, as
:mod:`alntools_amd.ecb_bus_correct` is.  The wrapper takes numpy arrays (the host entry point) or CUDA tensors (the ``_device`` one)
through :mod:`alntools_amd.ecb`'s one array kind.  The host-side helpers of the option live here too: which tag means what
(:func:`parse_tag`) and where a batch of records may be cut (:func:`cut_whole_reads`)."""
from __future__ import annotations

import ctypes as C
import re

import numpy as np

from . import ecb
from .ecb import _P, _int, _kind, _sig, _u32, _u64, _vp

STRATA_SYMBOLS = ("ecb_best_strata_device", "ecb_best_strata")

#: rows as in :data:`alntools_amd.ecb.SIGNATURES`
STRATA_SIGNATURES = (
    _sig("ecb_best_strata", [_int, _vp, _vp, _vp, _u64, _u32, _vp, _vp, _P(_u64)], twin=True),
)

FLAG_STRATA_DROPPED = 0x4000       # include/ecb_strata.h: ECB_FLAG_STRATA_DROPPED
LOWEST, HIGHEST = 0, 1             # ECB_STRATA_LOWEST, ECB_STRATA_HIGHEST

#: ``--best-strata TAG``: TAG -> (the tag read, the tag added to it where a record has it, whether the lowest score is the best)
TAGS = {"NM": ("NM", None, True), "XM": ("XM", None, True), "nM": ("nM", None, True), "AS": ("AS", None, False),
        "AS+YS": ("AS", "YS", False)}

_REFUSAL = re.compile(r"strata: record (\d+): ")


class StrataContractError(ecb.TupleContractError):
    """``ecb_best_strata`` refused its stream: ``record`` is the lowest offending record (0-based)."""


def parse_tag(tag):
    """``(tag_a, tag_b or None, lowest)`` of a ``--best-strata`` argument; anything but :data:`TAGS` is a ``ValueError``."""
    if tag not in TAGS:
        raise ValueError("--best-strata %s: the tag is one of %s" % (tag, ", ".join(TAGS)))
    return TAGS[tag]


def cut_whole_reads(read_id, final=False):
    """Where a batch whose open read is carried over may be cut: the number of leading records that are whole reads -- everything
    before the last step of ``read_id`` (the records from there on are the read still open, and go with the next batch), or all of
    them when ``final``.  0: the batch holds no read boundary."""
    n = len(read_id)
    if final or n == 0:
        return n
    step = np.flatnonzero(read_id[1:] != read_id[:-1])
    return int(step[-1]) + 1 if len(step) else 0


def load():
    """:func:`alntools_amd.ecb.load`'s library with this module's entry points bound (a library that lacks one fails here)."""
    return ecb.bind(STRATA_SIGNATURES)


def best_strata(read_id, hapflag, score, lowest=True, device=0, inplace=False):
    """bowtie's ``--best --strata`` over a tuple stream, on the GPU (``ecb_best_strata`` / ``ecb_best_strata_device``): of every read's
    passing records those with the best ``score`` (int32; the lowest, or the highest with ``lowest=False``) are kept, the others get
    ``hapflag | 0x4 | 0x4000``, and the records before a read's first kept one carry the read before's id.  ``read_id`` / ``hapflag``:
    uint32 arrays, or int32 tensors holding the same bytes; whole reads.  ``inplace``: the two arrays handed in are overwritten and
    returned (they must then be contiguous and of those types).  Returns ``(read_id, hapflag, counts)`` of the same kind; ``counts`` is
    the tuple ``(passing, kept, dropped, reads whose first passing record was dropped)``.  A stream that breaks the contract raises
    :class:`StrataContractError` with the lowest offender's index; everything else :class:`alntools_amd.ecb.EcbError`."""
    lib = load()
    k = _kind(read_id, device)
    p = k.ptr
    rid, hf, sc = k.words(read_id), k.words(hapflag), k.arr(score, k.i32)
    n = len(rid)
    if len(hf) != n or len(sc) != n:
        raise ValueError("read_id, hapflag and score hold %d, %d and %d records" % (n, len(hf), len(sc)))
    k.ready()
    if inplace:
        if rid is not read_id or hf is not hapflag:
            raise ValueError("inplace needs contiguous %s arrays" % ("int32" if k.tensors else "uint32"))
        out_rid, out_hf = rid, hf
    else:
        out_rid, out_hf = k.empty(max(n, 1), k.u32), k.empty(max(n, 1), k.u32)
    counts = (C.c_uint64 * 4)()
    rc = k.entry(lib, "ecb_best_strata")(k.device, p(rid), p(hf), p(sc), n, LOWEST if lowest else HIGHEST, p(out_rid), p(out_hf), counts)
    ecb._check_offender(lib, rc, _REFUSAL, StrataContractError)
    return out_rid, out_hf, tuple(int(x) for x in counts)            # (n = 0 is refused: the outputs hold n records)
