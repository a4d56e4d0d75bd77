# -*- coding: utf-8 -*-
"""ecclusters' bindings: ``ecb_components`` / ``ecb_components_device`` of ``libecb.so`` (``include/ecb_components.h``), bound lazily on the
library :func:`alntools_amd.ecb.load` returns, with a symbol tuple and a signature table of their own.  The wrapper takes numpy arrays
(the host entry point) or CUDA tensors (the ``_device`` one) through :mod:`alntools_amd.ecb`'s one array kind."""
from __future__ import annotations

import ctypes as C

from . import ecb
from .ecb import _A_N, _P, _check, _i64, _kind, _matrices, _sig, _u64, _vp

COMPONENTS_SYMBOLS = ("ecb_components_device", "ecb_components")

#: rows as in :data:`alntools_amd.ecb.SIGNATURES`
COMPONENTS_SIGNATURES = (
    _sig("ecb_components", _A_N + [_i64, _i64] + [_vp] * 5 + [_P(_u64)], twin=True),
)

def load():
    """:func:`alntools_amd.ecb.load`'s library with this module's entry points bound (a library that lacks one fails here)."""
    return ecb.bind(COMPONENTS_SIGNATURES)


def components(indptr, indices, data, n_loci, n_haps, indptr_n, indices_n, data_n, sample=None, min_count=1, device=0):
    """The connected components of the target-EC incidence on the GPU (``ecb_components`` / ``ecb_components_device``): the loci that the
    rows of CSR A tie together, a row counting when its weight -- count-alignments' ``w[e]``: its row sum of CSC N, or its entry in column
    ``sample`` -- reaches ``min_count`` and it has a column whose mask is not 0.  Components are numbered by their smallest locus.
    Returns ``(comp_of_locus int32 [T], comp_of_ec int32 [E] (-1: the row links nothing), comp_loci int32 [C], comp_ecs int32 [C],
    comp_reads int64 [C], sizes)`` of the same kind as the input; ``sizes`` is the tuple ``(C, linking rows, loci of the largest component,
    components with two loci or more)``.  Malformed input, an unknown sample or a negative ``min_count`` raises :class:`EcbError`."""
    lib = load()
    k = _kind(indptr, device)
    p = k.ptr
    s = -1 if sample is None else int(sample)
    (ip, ix, da, pn, xn, dn), (E, nnz, S, nnz_n) = _matrices(k, (indptr, indices, data, indptr_n, indices_n, data_n))
    k.ready()
    T = int(n_loci)
    of_locus, of_ec = k.empty(T, k.i32), k.empty(E, k.i32)
    loci, ecs, reads = k.empty(T, k.i32), k.empty(T, k.i32), k.empty(T, k.i64)
    sizes = (C.c_uint64 * 4)()
    _check(lib, k.entry(lib, "ecb_components")(k.device, E, T, n_haps, nnz, p(ip), p(ix), p(da), S, nnz_n, p(pn), p(xn), p(dn), s, int(min_count),
                                               p(of_locus), p(of_ec), p(loci), p(ecs), p(reads), sizes))
    n = int(sizes[0])
    return of_locus, of_ec, loci[:n], ecs[:n], reads[:n], tuple(int(v) for v in sizes)
