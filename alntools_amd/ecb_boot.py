# -*- coding: utf-8 -*-
"""ecboot's bindings: ``ecb_resample*`` and ``ecb_quantify_bootstrap*`` of ``libecb.so`` (``include/ecb_quant_boot.h``), bound lazily on the
library :func:`alntools_amd.ecb.load` returns, with a symbol tuple and a signature table of their own.  Both wrappers take numpy arrays
(the host entry points) or CUDA tensors (the ``_device`` ones) through :mod:`alntools_amd.ecb`'s one array kind."""
from __future__ import annotations

import ctypes as C

from . import ecb
from .ecb import _A_N, _P, _check, _check_gene, _check_tables, _dbl, _i64, _int, _kind, _matrices, _sig, _u32, _u64, _vp

BOOT_SYMBOLS = ("ecb_resample_device", "ecb_resample", "ecb_quantify_bootstrap_device", "ecb_quantify_bootstrap")

#: rows as in :data:`alntools_amd.ecb.SIGNATURES`
BOOT_SIGNATURES = (
    _sig("ecb_resample", [_int, _u32, _u32, _u64, _vp, _vp, _vp, _i64, _u64, _u64, _u32, _vp, _vp, _vp, _u64, _P(_u64)], twin=True),
    _sig("ecb_quantify_bootstrap", _A_N + [_i64, _vp, _u32, _dbl, _u64, _u32, _vp, _u32, _u64, _u32] + [_vp] * 9, twin=True),
)

def load():
    """:func:`alntools_amd.ecb.load`'s library with this module's entry points bound (a library that lacks one fails here)."""
    return ecb.bind(BOOT_SIGNATURES)


def resample(n_ecs, indptr_n, indices_n, data_n, sample=None, seed=0, b0=0, n_reps=1, device=0):
    """Bootstrap replicates of CSC N on the GPU (``ecb_resample`` / ``ecb_resample_device``): replicates ``b0 .. b0 + n_reps - 1`` of the
    ``W`` reads of column ``sample`` (None: all columns pooled), redrawn with replacement by Philox4x32-10 under ``seed`` -- a function of
    ``(N, sample, seed, b)`` alone.  Returns ``(rep_ptr int32 [n_reps + 1], rep_ec int32 [nnz], rep_count int32 [nnz])`` of the same kind
    as the input: a CSC N of ``n_reps`` columns that every other call takes as a multisample N.  A count-only call sizes the arrays first."""
    lib = load()
    k = _kind(indptr_n, device)
    p, fn = k.ptr, k.entry(lib, "ecb_resample")
    pn, xn, dn = (k.arr(a, k.i32) for a in (indptr_n, indices_n, data_n))
    if len(xn) != len(dn):
        raise ValueError("indices and data differ in length")
    k.ready()
    s = -1 if sample is None else int(sample)
    head = (k.device, int(n_ecs), len(pn) - 1, len(xn), p(pn), p(xn), p(dn), s, int(seed), int(b0), int(n_reps))
    nnz = C.c_uint64()
    rep_ptr = k.empty(int(n_reps) + 1, k.i32)
    _check(lib, fn(*(head + (p(rep_ptr), None, None, 0, C.byref(nnz)))))        # (the size first ...
    rep_ec, rep_count = k.empty(nnz.value, k.i32), k.empty(nnz.value, k.i32)
    if nnz.value:
        _check(lib, fn(*(head + (p(rep_ptr), p(rep_ec), p(rep_count), nnz.value, C.byref(nnz)))))      # ... then the entries, into arrays that fit)
    return rep_ptr, rep_ec, rep_count


def quantify_bootstrap(indptr, indices, data, n_loci, n_haps, indptr_n, indices_n, data_n, n_reps, seed=0, sample=None, scale=None, max_iters=1000,
                       tol=1e-6, budget_bytes=0, gene=None, n_genes=0, model=4, device=0, return_reps=False):
    """ecboot on the GPU (``ecb_quantify_bootstrap`` / ``ecb_quantify_bootstrap_device``): replicate ``b < n_reps`` is replicate ``b`` of
    :func:`resample` quantified as a cell of :func:`alntools_amd.ecb.quantify_cells` (``model`` 4) or ``quantify_cells_model`` (``gene``,
    ``n_genes``, ``model`` 1..3) would be; the mean and the standard deviation (``B - 1`` below the root) of the dense estimates per
    ``(h, t)`` and of their sums over ``h``.  Returns ``(mean[H, T], sd[H, T], tot_mean[T], tot_sd[T], info[, reps[B, H, T]])``, float64 of the
    same kind as the input; ``info`` is a dict of per-replicate arrays ``n_iter``, ``delta``, ``explained`` and ``converged`` as
    ``quantify_cells`` returns them per cell.  The result does not depend on ``budget_bytes``."""
    lib = load()
    k = _kind(indptr, device)
    p = k.ptr
    (ip, ix, da, pn, xn, dn), (E, nnz, S, nnz_n) = _matrices(k, (indptr, indices, data, indptr_n, indices_n, data_n))
    sc, gn = k.arr(scale, k.f64), k.arr(gene, k.i32)
    _check_tables((sc,), n_loci, n_haps, "scale")
    _check_gene(gn, n_loci)
    k.ready()
    B = int(n_reps)
    s = -1 if sample is None else int(sample)
    mean, sd = k.empty((n_haps, n_loci), k.f64), k.empty((n_haps, n_loci), k.f64)
    tm, ts = k.empty(n_loci, k.f64), k.empty(n_loci, k.f64)
    reps = k.empty((B, n_haps, n_loci), k.f64) if return_reps else None
    it, dl, ex, cv = k.empty(B, k.u32), k.empty(B, k.f64), k.empty(B, k.i64), k.empty(B, k.u8)
    _check(lib, k.entry(lib, "ecb_quantify_bootstrap")(
        k.device, E, n_loci, n_haps, nnz, p(ip), p(ix), p(da), S, nnz_n, p(pn), p(xn), p(dn), s, p(sc), int(max_iters), float(tol), int(budget_bytes),
        int(n_genes), p(gn), int(model), int(seed), B, p(mean), p(sd), p(tm), p(ts), p(reps), p(it), p(dl), p(ex), p(cv)))
    if k.tensors:                                    # (the uint32 the library wrote, in a type torch computes with)
        it = it.to(k.i64).bitwise_and(0xFFFFFFFF)
    info = {"n_iter": it, "delta": dl, "explained": ex, "converged": cv != 0}
    return (mean, sd, tm, ts, info) + ((reps,) if return_reps else ())
