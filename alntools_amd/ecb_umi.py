# -*- coding: utf-8 -*-
"""``--collapse-umis``'s bindings: ``ecb_collapse_umis`` / ``ecb_collapse_umis_device`` of ``libecb.so`` (``include/ecb_umi.h``), bound
lazily on the library :func:`alntools_amd.ecb.load` returns, with a symbol tuple and a signature table of their own, as
:mod:`alntools_amd.ecb_strata` is.  The wrapper takes numpy arrays (the host entry point) or CUDA tensors (the ``_device`` one) through
:mod:`alntools_amd.ecb`'s one array kind.  The host-side helpers of the option live here too: a UMI's code (:func:`pack_umi`) and a
read's molecule key (:func:`mol_keys`)."""
from __future__ import annotations

import ctypes as C
import re

import numpy as np

from . import ecb
from .ecb import _P, _int, _kind, _sig, _u32, _u64, _vp

UMI_SYMBOLS = ("ecb_collapse_umis_device", "ecb_collapse_umis")

#: rows as in :data:`alntools_amd.ecb.SIGNATURES`
UMI_SIGNATURES = (
    _sig("ecb_collapse_umis", [_int, _vp, _vp, _vp, _vp, _u64, _u64, _u32, _u32, _vp, _vp, _vp, _vp, _P(_u64)], twin=True),
)

UMI_NONE = 0xFFFFFFFFFFFFFFFF      # include/ecb_umi.h: ECB_UMI_NONE
MAX_UMILEN = 16                    # bases a code holds: 2 bits each behind a leading 1 bit, 33 bits under the cell id
CELL_SHIFT = 33                    # mol_key = cell id << CELL_SHIFT | pack_umi(...)
MAX_RECORDS = (1 << 30) - 1        # include/ecb_umi.h: n < 2^30
COUNT_NAMES = ("reads in", "molecules", "molecules of several reads", "molecules discarded", "records out", "reads without a UMI")

_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
_REFUSAL = re.compile(r"umi: record (\d+): ")


class UmiContractError(ecb.TupleContractError):
    """``ecb_collapse_umis`` refused its stream: ``record`` is the lowest offending record (0-based)."""


def pack_umi(text):
    """A UMI's code: 2 bits per base (A, C, G, T = 0 .. 3, the first base highest) behind a leading 1 bit, so that UMIs of different
    lengths differ; 1 to 16 upper-case bases.  Anything else -- an empty field, another letter such as ``N``, lower case, more than 16
    bases, no string -- is None: the read then joins no molecule."""
    if isinstance(text, bytes):
        try:
            text = text.decode("ascii")
        except UnicodeDecodeError:
            return None
    if not isinstance(text, str) or not 1 <= len(text) <= MAX_UMILEN:
        return None
    code = 1
    for ch in text:
        v = _CODE.get(ch)
        if v is None:
            return None
        code = code << 2 | v
    return code


def mol_keys(cell_ids, umis):
    """uint64 molecule keys of reads: ``cell id << 33 | pack_umi(umi)``, :data:`UMI_NONE` where the field is no UMI."""
    out = np.full(len(umis), UMI_NONE, dtype=np.uint64)
    cache = {}
    for i, (c, u) in enumerate(zip(cell_ids, umis)):
        code = cache.get(u, -1)
        if code == -1:
            code = cache[u] = pack_umi(u)
        if code is not None:
            out[i] = (int(c) << CELL_SHIFT) | code
    return out


def load():
    """:func:`alntools_amd.ecb.load`'s library with this module's entry points bound (a library that lacks one fails here)."""
    return ecb.bind(UMI_SIGNATURES)


def collapse_umis(read_id, locus, hapflag, mol_key, n_loci, n_haps, device=0):
    """The reads of one molecule made one read, on the GPU (``ecb_collapse_umis`` / ``ecb_collapse_umis_device``; the rule:
    ``include/ecb_umi.h``).  ``read_id`` / ``locus`` / ``hapflag``: uint32 arrays, or int32 tensors holding the same bytes; whole reads.
    ``mol_key``: one uint64 (int64 in a tensor) per read of the stream; reads with equal keys are one molecule, :data:`UMI_NONE` joins
    nothing.  Returns ``(read_id, locus, hapflag, first_read, counts)`` of the same kind: the collapsed stream, ids from 0; the first
    read of every surviving molecule, 0-based; ``counts`` the tuple :data:`COUNT_NAMES` names.  A stream that breaks the contract, or
    holds other than ``len(mol_key)`` reads, raises :class:`UmiContractError` with the lowest offender's index; everything else
    :class:`alntools_amd.ecb.EcbError`."""
    lib = load()
    k = _kind(read_id, device)
    p = k.ptr
    rid, loc, hf = (k.words(a) for a in (read_id, locus, hapflag))
    key = k.words(mol_key, 64)
    n, n_reads = len(rid), len(key)
    if len(loc) != n or len(hf) != n:
        raise ValueError("read_id, locus and hapflag hold %d, %d and %d records" % (n, len(loc), len(hf)))
    if not n_reads:
        key = k.empty(1, k.u64)                                  # (a stream of no read: still a pointer)
    k.ready()
    out = [k.empty(max(n, 1), k.u32) for _ in range(3)]
    first = k.empty(max(n_reads, 1), k.u32)
    counts = (C.c_uint64 * 6)()
    rc = k.entry(lib, "ecb_collapse_umis")(k.device, p(rid), p(loc), p(hf), p(key), n, n_reads, n_loci, n_haps, p(out[0]), p(out[1]), p(out[2]),
                                           p(first), counts)
    ecb._check_offender(lib, rc, _REFUSAL, UmiContractError)
    c = tuple(int(x) for x in counts)
    return out[0][:c[4]], out[1][:c[4]], out[2][:c[4]], first[:c[1] - c[3]], c
