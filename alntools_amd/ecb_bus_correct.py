# -*- coding: utf-8 -*-
"""Barcode correction's bindings: ``ecb_bus_correct`` / ``ecb_bus_correct_device`` of ``libecb.so`` (``include/ecb_bus_correct.h``), bound
lazily on the library :func:`alntools_amd.ecb.load` returns, with a symbol tuple and a signature table of their own, as
:mod:`alntools_amd.ecb_bus` is.  The wrapper takes numpy arrays (the host entry point) or CUDA tensors (the ``_device`` one) through
:mod:`alntools_amd.ecb`'s one array kind."""
from __future__ import annotations

import ctypes as C
import re

from . import ecb
from .ecb import _P, _int, _kind, _sig, _u32, _u64, _vp
from .ecb_bus import RECORD_BYTES, BusFormatError

BUS_CORRECT_SYMBOLS = ("ecb_bus_correct_device", "ecb_bus_correct")

#: rows as in :data:`alntools_amd.ecb.SIGNATURES`
BUS_CORRECT_SIGNATURES = (
    _sig("ecb_bus_correct", [_int, _vp, _u64, _u32, _vp, _u64, _u64, _vp, _vp, _P(_u64)], twin=True),
)

EXACT, CORRECTED, NO_CANDIDATE, AMBIGUOUS = 0, 1, 2, 3      # include/ecb_bus_correct.h: ECB_BUS_EXACT ..., and the order of the sizes

_REFUSAL = re.compile(r"bus: (record|whitelist entry) (\d+): ")


class WhitelistFormatError(BusFormatError):
    """``ecb_bus_correct`` refused its whitelist: ``what`` is ``"whitelist entry"``, ``index`` the lowest offending entry (0-based)."""


def _refusal(code, msg, what, index):
    return (BusFormatError if what == "record" else WhitelistFormatError)(code, msg, what, index)


def load():
    """:func:`alntools_amd.ecb.load`'s library with this module's entry points bound (a library that lacks one fails here)."""
    return ecb.bind(BUS_CORRECT_SIGNATURES)


def correct(records, bclen, whitelist, want_status=False, capacity=None, device=0):
    """bustools correct's rule on the GPU (``ecb_bus_correct`` / ``ecb_bus_correct_device``).  ``records``: the BUS file's records as they
    lie in it, ``n x 32`` bytes (a uint8 array or tensor); ``whitelist``: uint64, strictly ascending, every value below ``4 ** bclen``.
    ``capacity``: the room for kept records, None: ``n``, the header's bound.  Returns ``(records_out uint8 [n_out, 32], status uint8 [n]
    or None, sizes)`` of the same kind as ``records``; ``sizes`` is the tuple ``(exact, corrected, without a candidate, ambiguous)`` and
    ``n_out`` its first two added.  A malformed record raises :class:`alntools_amd.ecb_bus.BusFormatError` (``what`` = ``"record"``), a
    malformed whitelist :class:`WhitelistFormatError` (``"whitelist entry"``), each with the lowest offender's index; everything else
    :class:`alntools_amd.ecb.EcbError`."""
    lib = load()
    k = _kind(records, device)
    p = k.ptr
    rec = k.bytes(records)
    if len(rec) % RECORD_BYTES:
        raise ValueError("the records are %d bytes: not a multiple of %d" % (len(rec), RECORD_BYTES))
    n = len(rec) // RECORD_BYTES
    wl = k.words(whitelist, 64)
    k.ready()
    cap = n if capacity is None else int(capacity)
    out = k.empty(max(cap, 1) * RECORD_BYTES, k.u8)
    status = k.empty(max(n, 1), k.u8) if want_status else None
    sizes = (C.c_uint64 * 4)()
    rc = k.entry(lib, "ecb_bus_correct")(k.device, p(rec), n, int(bclen), p(wl), len(wl), cap, p(out), p(status), sizes)
    ecb._check_offender(lib, rc, _REFUSAL, _refusal)
    sizes = tuple(int(x) for x in sizes)
    n_out = sizes[0] + sizes[1]
    return out[:n_out * RECORD_BYTES].reshape(n_out, RECORD_BYTES), (None if status is None else status[:n]), sizes
