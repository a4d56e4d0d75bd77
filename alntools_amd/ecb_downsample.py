# -*- coding: utf-8 -*-
"""ecdownsample's bindings: ``ecb_downsample`` / ``ecb_downsample_device`` of ``libecb.so`` (``include/ecb_downsample.h``), bound lazily on
the library :func:`alntools_amd.ecb.load` returns, with a symbol tuple and a signature table of their own, as :mod:`alntools_amd.ecb_umi`
is.  The wrapper takes numpy arrays (the host entry point) or CUDA tensors (the ``_device`` one) through :mod:`alntools_amd.ecb`'s one
array kind."""
from __future__ import annotations

from . import ecb
from .ecb import _check, _int, _kind, _sig, _u32, _u64, _vp

DOWNSAMPLE_SYMBOLS = ("ecb_downsample_device", "ecb_downsample")

#: rows as in :data:`alntools_amd.ecb.SIGNATURES`
DOWNSAMPLE_SIGNATURES = (
    _sig("ecb_downsample", [_int, _u32, _u32, _u64, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp], twin=True),
)

MAX_READS = (1 << 31) - 1          # include/ecb_downsample.h: a thinned sample holds fewer than 2^31 reads


def load():
    """:func:`alntools_amd.ecb.load`'s library with this module's entry points bound (a library that lacks one fails here)."""
    return ecb.bind(DOWNSAMPLE_SIGNATURES)


def downsample(indptrN, indicesN, dataN, n_ecs, target, seed=0, device=0):
    """``target[s]`` of the reads of every sample ``s`` of CSC N kept, drawn without replacement on the GPU (``ecb_downsample`` /
    ``ecb_downsample_device``; the rule: ``include/ecb_downsample.h``).  ``target``: one int64 per sample; below 0, or at or above the
    sample's reads: the column is copied; 0: it is emptied.  The draw is a function of ``(N, target, seed)`` alone, and a sample's result
    does not depend on the other samples' targets.  Returns ``(dataN_out, in_total, out_total)`` of the same kind as the input: int32
    counts, one per entry of N at the entry's own place (zeros included: ``indptrN`` and ``indicesN`` stay valid), and int64 reads per
    sample before and after.  Malformed input raises :class:`alntools_amd.ecb.EcbError` (``ECB_ERR_CONTRACT``), a thinned sample of 2^31
    reads or more ``ECB_ERR_LIMIT``."""
    lib = load()
    k = _kind(indptrN, device)
    p = k.ptr
    pn, xn, dn = (k.arr(a, k.i32) for a in (indptrN, indicesN, dataN))
    tg = k.arr(target, k.i64)
    S, nnz = len(pn) - 1, len(xn)
    if len(dn) != nnz:
        raise ValueError("indices and data differ in length")
    if len(tg) != S:
        raise ValueError("target has %d entries for %d samples" % (len(tg), S))
    if not S:
        tg = k.arr([0], k.i64)                                   # (no sample: still a pointer)
    k.ready()
    out, tin, tout = k.empty(max(nnz, 1), k.i32), k.empty(max(S, 1), k.i64), k.empty(max(S, 1), k.i64)
    _check(lib, k.entry(lib, "ecb_downsample")(k.device, int(n_ecs), S, nnz, p(pn), p(xn), p(dn), p(tg), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                               p(out), p(tin), p(tout)))
    return out[:nnz], tin[:S], tout[:S]
