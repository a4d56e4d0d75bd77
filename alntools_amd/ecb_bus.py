# -*- coding: utf-8 -*-
"""bus2ec's bindings: ``ecb_bus_molecules`` / ``ecb_bus_molecules_device`` of ``libecb.so`` (``include/ecb_bus.h``), bound lazily on the
library :func:`alntools_amd.ecb.load` returns, with a symbol tuple and a signature table of their own.  The wrapper takes numpy arrays
(the host entry point) or CUDA tensors (the ``_device`` one) through :mod:`alntools_amd.ecb`'s one array kind."""
from __future__ import annotations

import ctypes as C
import re

import numpy as np

from . import ecb
from .ecb import _P, _int, _kind, _sig, _u32, _u64, _vp

BUS_SYMBOLS = ("ecb_bus_molecules_device", "ecb_bus_molecules")

#: rows as in :data:`alntools_amd.ecb.SIGNATURES`
BUS_SIGNATURES = (
    _sig("ecb_bus_molecules", [_int, _vp, _u64, _u32, _u32, _u32, _u32, _u64, _vp, _vp, _u32, _vp, _vp, _u32, _u32, _vp, _u64] + [_u64] * 4 + [_vp] * 8
         + [_P(_u64)], twin=True),
)

NO_UMI = 1                 # include/ecb_bus.h: ECB_BUS_NO_UMI
MAX_UMILEN = 16            # include/ecb_bus.h: ECB_BUS_MAX_UMILEN
RECORD_BYTES = 32

_REFUSAL = re.compile(r"bus: (?:matrix\.ec )?(record|line) (\d+): ")


class BusFormatError(ecb.OffenderError):
    """``ecb_bus_molecules`` refused its input: ``what`` is ``"record"`` or ``"line"``, ``index`` the lowest offender (0-based)."""


def load():
    """:func:`alntools_amd.ecb.load`'s library with this module's entry points bound (a library that lacks one fails here)."""
    return ecb.bind(BUS_SIGNATURES)


def a_capacity(records, ec_ptr):
    """The header's bound on A's non-zeros: the sum over the records of the length of their EC's line (host arrays; ec fields out of range
    count as the longest line: the library refuses them before it writes)."""
    ptr = np.asarray(ec_ptr, dtype=np.int64)
    lens = np.diff(ptr)
    if not len(lens) or not len(records):
        return 0
    ec = np.ascontiguousarray(records).view(np.uint8).reshape(-1, RECORD_BYTES)[:, 16:20].copy().view('<i4').reshape(-1)
    return int(np.maximum(lens, 0)[np.clip(ec, 0, len(lens) - 1)].sum())


def molecules(records, bclen, umilen, ec_ptr, ec_targets, target_col, target_hap, n_loci, n_haps, keep=None, no_umi=False, capacities=None, device=0):
    """bustools count's rule for EC matrices on the GPU (``ecb_bus_molecules`` / ``ecb_bus_molecules_device``).  ``records``: the BUS
    file's records as they lie in it, ``n x 32`` bytes (a uint8 array or tensor); ``ec_ptr`` / ``ec_targets``: ``matrix.ec`` as a CSR over
    target ids; ``target_col`` / ``target_hap``: every target's column and haplotype; ``keep``: the barcodes to keep, uint64, strictly
    ascending (None: all).  ``capacities``: (cells, rows, nnz_a, nnz_n), None: the header's bounds.  Returns ``(barcodes uint64 [cells],
    (indptrA, indicesA, dataA), (indptrN, indicesN, dataN), row_line int32 [rows], sizes)`` of the same kind as ``records`` (tensors carry
    the barcodes as int64: the same bytes); ``sizes`` is the tuple ``(cells, rows, nnz_a, nnz_n, molecules, molecules of several ECs,
    molecules discarded, new rows)``.  Malformed input raises :class:`BusFormatError` naming the lowest offending record or line; limits
    raise :class:`EcbError`."""
    lib = load()
    k = _kind(records, device)
    p = k.ptr
    rec = k.bytes(records)
    if len(rec) % RECORD_BYTES:
        raise ValueError("the records are %d bytes: not a multiple of %d" % (len(rec), RECORD_BYTES))
    n = len(rec) // RECORD_BYTES
    if k.tensors:                                    # what differs: a tensor is made of the ids as int64 (torch takes no uint32 array everywhere)
        ec_ptr, ec_targets, target_col, target_hap = (a if hasattr(a, "data_ptr") else np.asarray(a, dtype=np.int64)
                                                      for a in (ec_ptr, ec_targets, target_col, target_hap))
    ptr, ids, tc, th = (k.arr(a, k.u32) for a in (ec_ptr, ec_targets, target_col, target_hap))
    kp = k.words(keep, 64)
    if len(tc) != len(th):
        raise ValueError("target_col and target_hap differ in length")
    k.ready()
    if capacities is None:
        host_ptr = ptr.cpu().numpy() if k.tensors else ptr
        host_rec = rec.cpu().numpy() if k.tensors else rec
        capacities = (n if kp is None else min(n, len(kp)), n, min(a_capacity(host_rec, host_ptr.view(np.uint32)), (1 << 31) - 1), n)
    cc, cr, ca, cn = (int(x) for x in capacities)
    out = [k.empty(max(cc, 1), k.u64), k.empty(cr + 1, k.i32), k.empty(max(ca, 1), k.i32), k.empty(max(ca, 1), k.i32), k.empty(cc + 1, k.i32),
           k.empty(max(cn, 1), k.i32), k.empty(max(cn, 1), k.i32), k.empty(max(cr, 1), k.i32)]
    sizes = (C.c_uint64 * 8)()
    rc = k.entry(lib, "ecb_bus_molecules")(k.device, p(rec), n, int(bclen), int(umilen), NO_UMI if no_umi else 0, len(ptr) - 1, len(ids), p(ptr), p(ids),
                                           len(tc), p(tc), p(th), int(n_loci), int(n_haps), p(kp), 0 if kp is None else len(kp), cc, cr, ca, cn,
                                           *([p(o) for o in out] + [sizes]))
    ecb._check_offender(lib, rc, _REFUSAL, BusFormatError)
    cells, rows, nnz_a, nnz_n = (int(x) for x in sizes[:4])
    return (out[0][:cells], (out[1][:rows + 1], out[2][:nnz_a], out[3][:nnz_a]), (out[4][:cells + 1], out[5][:nnz_n], out[6][:nnz_n]), out[7][:rows],
            tuple(int(x) for x in sizes))
