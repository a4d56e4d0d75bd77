# -*- coding: utf-8 -*-
"""ctypes binding of ``libecb.so`` (``include/ecb.h``) -- the device side of the
reference's ``process_convert_bam`` + merge + A/N construction
(``alntools/bam_utils.py:198-363, 680-724, 768-847``).

There is no CPU fallback here on purpose: if the library is missing or no GPU is
present, constructing an :class:`EcBuilder` raises.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, os.environ.get("ECB_LIB", "libecb.so"))   # ECB_LIB: A/B builds of the kernel

F_RANGES = 1
F_MULTISAMPLE = 2
F_VERIFY = 4
HAP_SHIFT = 16
FLAG_MATE_OTHER_REF = 0x1000
FLAG_NEXT_POS_NEG = 0x2000

#: every symbol include/ecb.h declares
SYMBOLS = ("ecb_abi_version", "ecb_device_count", "ecb_create", "ecb_destroy", "ecb_reset", "ecb_last_error",
           "ecb_push", "ecb_push_device", "ecb_hint_reads", "ecb_push_cells", "ecb_push_cells_device", "ecb_verify_device", "ecb_finalize", "ecb_export",
           "ecb_export_device", "ecb_export_ranges", "ecb_export_range_minmax", "ecb_export_pairs", "ecb_ms_filter", "ecb_ms_export",
           "ecb_export_read_ec", "ecb_table_sizes",
           "ecb_table_export_device", "ecb_table_merge_device", "ecb_table_export_parts_device",
           "ecb_table_adopt_device", "ecb_table_merge_batch_device", "ecb_table_adopt_batch_device",
           "ecb_export_firsts_device", "ecb_assemble_ranges_device", "ecb_table_rebase_device",
           "ecb_export_ec_keys_device", "ecb_ms_local_triples_device", "ecb_ms_adopt_triples_device", "ecb_counters", "ecb_add_counters", "ecb_profile",
           "ecb_profile_read", "ecb_profile_kernel", "ecb_csr_to_hapcsc_device", "ecb_hapcsc_to_csr_device", "ecb_release_scratch",
           "ecb_csr_to_hapcsc", "ecb_hapcsc_to_csr", "ecb_merge", "ecb_push_device_tiled", "ecb_verify_device_tiled",
           "ecb_apply_mask_device", "ecb_apply_mask", "ecb_combine_device", "ecb_combine",
           "ecb_salmon_ecs_device", "ecb_salmon_ecs")
#: every symbol include/ecb_count.h declares (ecb.h includes it)
COUNT_SYMBOLS = ("ecb_count_alignments_device", "ecb_count_alignments")
#: every symbol include/ecb_bundle.h declares (ecb.h includes it)
BUNDLE_SYMBOLS = ("ecb_bundle_device", "ecb_bundle")
#: every symbol include/ecb_select.h declares (ecb.h includes it)
SELECT_SYMBOLS = ("ecb_select_device", "ecb_select")
#: every symbol include/ecb_quant.h declares (ecb.h includes it)
QUANT_SYMBOLS = ("ecb_quantify_device", "ecb_quantify")
#: every symbol include/ecb_quant_model.h declares (ecb_quant.h includes it)
QUANT_MODEL_SYMBOLS = ("ecb_quantify_model_device", "ecb_quantify_model")
#: every symbol include/ecb_quant_cells.h declares (ecb_quant.h includes it)
QUANT_CELLS_SYMBOLS = ("ecb_cell_support_device", "ecb_cell_support", "ecb_quantify_cells_device", "ecb_quantify_cells")
#: every symbol include/ecb_quant_cells_model.h declares (ecb_quant.h includes it)
QUANT_CELLS_MODEL_SYMBOLS = ("ecb_quantify_cells_model_device", "ecb_quantify_cells_model")
#: every symbol include/ecb_quant_post.h declares (ecb_quant.h includes it)
QUANT_POST_SYMBOLS = ("ecb_posterior_device", "ecb_posterior", "ecb_csr_to_hapcsc_values_device", "ecb_csr_to_hapcsc_values")
#: ``ecb_select``'s row classes (include/ecb_select.h)
ROW_CLASSES = {None: 0, "all": 0, "unique": 1, "locus-unique": 2, "multi": 3}
ABI_VERSION = 4            # include/ecb.h: ECB_ABI_VERSION
ECB_ERR_CONTRACT = -5      # include/ecb.h


class EcbError(RuntimeError):
    def __init__(self, code, msg):
        RuntimeError.__init__(self, "libecb error %d: %s" % (code, msg))
        self.code = code


class OffenderError(EcbError):
    """A refusal that names the lowest offender: ``what`` it is (``"record"``, ``"line"`` ...), ``index`` its 0-based number (``record``:
    the same).  The entry points' own errors derive from it."""

    def __init__(self, code, msg, what, index):
        EcbError.__init__(self, code, msg)
        self.what, self.index = what, index

    record = property(lambda self: self.index)


class TupleContractError(OffenderError):
    """A tuple stream refused: ``record`` is the lowest offending record (0-based)."""

    def __init__(self, code, msg, record):
        OffenderError.__init__(self, code, msg, "record", record)


def _check(lib, rc, h=None):
    """Raise :class:`EcbError` for a non-zero return code of libecb, with the message of handle ``h`` (None: of the last call without one)."""
    if rc != 0:
        raise EcbError(rc, (lib.ecb_last_error(h) or b"").decode())


def _check_offender(lib, rc, pattern, error):
    """:func:`_check` for a call without a handle whose ``ECB_ERR_CONTRACT`` names a lowest offender: where the message matches the
    compiled ``pattern``, ``error(rc, msg, *groups)`` is raised, the groups of digits as ints (``error``: an :class:`OffenderError`
    class, or a function that picks one); everything else is an :class:`EcbError`."""
    if rc != 0:
        msg = (lib.ecb_last_error(None) or b"").decode()
        m = pattern.match(msg) if rc == ECB_ERR_CONTRACT else None
        if m is None:
            raise EcbError(rc, msg)
        raise error(rc, msg, *(int(g) if g.isdigit() else g for g in m.groups()))


class Config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("n_loci", C.c_uint32),
                ("n_haplotypes", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32),
                ("ec_capacity", C.c_uint64), ("arena_capacity", C.c_uint64),
                ("max_batch_records", C.c_uint64)]


class Sizes(C.Structure):
    _fields_ = [("n_ecs", C.c_uint64), ("nnz_a", C.c_uint64), ("n_samples", C.c_uint64),
                ("nnz_n", C.c_uint64), ("all_alignments", C.c_uint64), ("valid_alignments", C.c_uint64),
                ("n_reads", C.c_uint64)]


class MsSizes(C.Structure):
    _fields_ = [("n_cells_seen", C.c_uint64), ("n_cells_kept", C.c_uint64), ("n_ecs_kept", C.c_uint64),
                ("nnz_a", C.c_uint64), ("nnz_n", C.c_uint64)]


class CombinePart(C.Structure):
    """``ecb_combine_part``: one input ``.bin`` of ``ecb_combine`` / ``ecb_combine_device``."""
    _fields_ = [("struct_size", C.c_uint32), ("n_ecs", C.c_uint32), ("n_samples", C.c_uint32), ("n_loci", C.c_uint32),
                ("nnz_a", C.c_uint64), ("nnz_n", C.c_uint64)] + [(n, C.c_void_p) for n in (
                    "indptr_a", "indices_a", "data_a", "indptr_n", "indices_n", "data_n", "target_map", "sample_map")]


_vp, _u64, _sz, _u32, _i64, _int, _dbl, _P = C.c_void_p, C.c_uint64, C.c_size_t, C.c_uint32, C.c_int64, C.c_int, C.c_double, C.POINTER
_HEAD = [_int, _u32, _u32, _u32]                                                  # device, n_ecs, n_loci, n_haps
_A_N = _HEAD + [_u64, _vp, _vp, _vp, _u32, _u64, _vp, _vp, _vp]                    # ... nnz, CSR A, n_samples, nnz_n, CSC N
_BATCH = [_vp, _u32, _P(_vp), _P(_u64), _P(_vp), _P(_u64)]
_INFO = [_P(_u32), _P(_dbl), _P(_i64), _P(_u32)]


def _sig(name, argtypes=None, restype=_int, twin=False, optional=False):
    """One row of :data:`SIGNATURES`.  ``twin``: ``name + "_device"`` has the same signature.  ``optional``: an A/B build named by
    ``ECB_LIB`` may lack it (a normal build may not)."""
    return name, argtypes, restype, twin, optional


#: what :func:`load` binds: (symbol, argtypes or None, restype, has a ``_device`` twin, optional under ``ECB_LIB``)
SIGNATURES = (
    _sig("ecb_abi_version"),
    _sig("ecb_device_count"),
    _sig("ecb_create", [_P(Config), _P(_vp)]),
    _sig("ecb_destroy", [_vp], restype=None),
    _sig("ecb_reset", [_vp]),
    _sig("ecb_last_error", [_vp], restype=C.c_char_p),
    _sig("ecb_push", [_vp, _vp, _vp, _vp, _vp, _sz], twin=True),
    _sig("ecb_hint_reads", [_vp, _u64]),
    _sig("ecb_push_cells", [_vp, _vp, _u64, _sz], twin=True),
    _sig("ecb_verify_device", [_vp, _vp, _vp, _vp, _sz, _P(_u64), _P(_u64)]),
    _sig("ecb_finalize", [_vp, _P(Sizes)]),
    _sig("ecb_export", [_vp] * 7, twin=True),
    _sig("ecb_export_ranges", [_vp, _vp]),
    _sig("ecb_export_read_ec", [_vp, _vp]),
    _sig("ecb_export_pairs", [_vp] * 5),
    _sig("ecb_export_range_minmax", [_vp, _vp, _vp]),
    _sig("ecb_ms_filter", [_vp, _u32, _i64, _P(MsSizes)]),
    _sig("ecb_ms_export", [_vp] * 8),
    _sig("ecb_table_sizes", [_vp, _P(_u64), _P(_u64), _P(_u64)]),
    _sig("ecb_table_export_device", [_vp, _vp, _vp, _u64]),
    _sig("ecb_table_merge_device", [_vp, _vp, _u64, _vp, _u64]),
    _sig("ecb_table_export_parts_device", [_vp, _vp, _vp, _u64, _u32, _P(_u64), _P(_u64)]),
    _sig("ecb_table_adopt_device", [_vp, _vp, _u64, _vp, _u64]),
    _sig("ecb_table_rebase_device", [_vp, _vp, _u64, _u64]),
    _sig("ecb_table_merge_batch_device", _BATCH),
    _sig("ecb_table_adopt_batch_device", _BATCH),
    _sig("ecb_export_ec_keys_device", [_vp, _vp]),
    _sig("ecb_export_firsts_device", [_vp, _vp]),
    _sig("ecb_assemble_ranges_device", [_vp, _u32] + [_P(_vp)] * 5 + [_P(_u64)] * 2 + [_u64, _u64, _u64, _P(Sizes)]),
    _sig("ecb_ms_local_triples_device", [_vp, _vp, _vp, _vp, _vp, _u64, _u64, _vp, _vp, _vp, _P(_u64)]),
    _sig("ecb_ms_adopt_triples_device", [_vp, _u32, _P(_vp), _P(_vp), _P(_vp), _P(_u64), _P(_u64)]),
    _sig("ecb_counters", [_vp, _P(_u64), _P(_u64), _P(_u64)]),
    _sig("ecb_add_counters", [_vp, _u64, _u64, _u64]),
    _sig("ecb_profile", [_vp, _int]),
    _sig("ecb_profile_read", [_vp, _P(_dbl), _P(_u64), _P(_u64)]),
    _sig("ecb_merge", [_P(_vp), _u32, _vp, _P(Sizes)], optional=True),
    _sig("ecb_push_device_tiled", [_vp, _vp, _sz], optional=True),
    _sig("ecb_verify_device_tiled", [_vp, _vp, _sz, _P(_u64), _P(_u64)], optional=True),
    _sig("ecb_profile_kernel", [_vp], restype=C.c_char_p, optional=True),
    _sig("ecb_csr_to_hapcsc", _HEAD + [_vp] * 5 + [_u64, _P(_u64)], optional=True),          # (the host entry point is told its room)
    _sig("ecb_csr_to_hapcsc_device", _HEAD + [_vp] * 5 + [_P(_u64)]),
    _sig("ecb_hapcsc_to_csr", _HEAD + [_vp, _vp, _u64, _vp, _vp, _vp, _P(_u64)], optional=True),
    _sig("ecb_hapcsc_to_csr_device", _HEAD + [_vp, _vp, _u64, _vp, _vp, _vp, _P(_u64)]),
    _sig("ecb_csr_to_hapcsc_values", _HEAD + [_vp] * 7 + [_u64, _P(_u64)], optional=True),
    _sig("ecb_csr_to_hapcsc_values_device", _HEAD + [_vp] * 7 + [_P(_u64)], optional=True),
    _sig("ecb_apply_mask", _HEAD + [_u64] + [_vp] * 7 + [_P(_u64)], twin=True, optional=True),
    _sig("ecb_combine", [_int, _u32, _P(CombinePart), _u32, _u32, _u32] + [_vp] * 6 + [_P(_u64)], twin=True, optional=True),
    _sig("ecb_salmon_ecs", [_int, _vp, _u64, _u32, _u32, _vp, _vp, _u32, _u32, _u64] + [_vp] * 5 + [_P(_u64)], twin=True, optional=True),
    _sig("ecb_count_alignments", _A_N + [_i64, _vp, _vp, _vp], twin=True, optional=True),
    _sig("ecb_bundle", [_int] + [_u32] * 5 + [_u64, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _u64, _vp, _vp, _u64] + [_vp] * 6 + [_P(_u64)],
         twin=True, optional=True),
    _sig("ecb_select", [_int] + [_u32] * 4 + [_u64, _vp, _vp, _vp, _u64, _vp, _vp, _vp, C.c_int32, _vp, _i64] + [_vp] * 7 + [_P(_u64)],
         twin=True, optional=True),
    _sig("ecb_quantify", _A_N + [_i64, _vp, _vp, _u32, _dbl, _vp] + _INFO, twin=True, optional=True),
    _sig("ecb_quantify_model", _A_N + [_i64, _vp, _vp, _u32, _dbl, _u32, _vp, _u32, _vp] + _INFO, twin=True, optional=True),
    _sig("ecb_cell_support", _A_N + [_vp, _vp, _vp, _u64, _P(_u64)], twin=True, optional=True),
    _sig("ecb_quantify_cells", _A_N + [_vp, _vp, _vp, _u32, _dbl, _u64, _u64] + [_vp] * 7, twin=True, optional=True),
    _sig("ecb_quantify_cells_model", _A_N + [_vp, _vp, _vp, _u32, _dbl, _u64, _u32, _vp, _u32, _u64] + [_vp] * 7, twin=True, optional=True),
    _sig("ecb_posterior", _HEAD + [_u64, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _u32, _u64, _vp, _vp, _vp], twin=True, optional=True),
)

_lib = None
_tables = {}        # id of a signature table -> the library object its rows were last bound on


def bind(signatures):
    """:func:`load`'s library with the rows of ``signatures`` (a table like :data:`SIGNATURES`) bound on it, once per library object.
    A symbol the library lacks fails here, unless the row is ``optional`` and ``ECB_LIB`` names the build."""
    lib = load()
    if _tables.get(id(signatures)) is not lib:
        _bind(lib, signatures)
    return lib


def _bind(lib, signatures):
    ab = "ECB_LIB" in os.environ        # (an A/B build named by hand, tools/: may be an older ABI; what it lacks is simply not bound)
    for name, argtypes, restype, twin, optional in signatures:
        for n in ((name + "_device", name) if twin else (name,)):
            if optional and ab and not hasattr(lib, n):
                continue
            f = getattr(lib, n)             # (a normal build that lacks one fails here)
            f.restype = restype
            if argtypes is not None:
                f.argtypes = argtypes
    _tables[id(signatures)] = lib


def load():
    """``ctypes.CDLL`` of the in-tree library (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64 (same SONAME as
    # /opt/rocm's).  Importing torch first makes the loader bind libecb's libamdhip64.so.7 to the copy
    # torch already mapped, so tensors and libecb share one runtime (two copies cannot both open the GPU).
    # A process that will never hold a tensor says so (ALNTOOLS_TORCH=0: the command line does, for its one-GPU commands --
    # everything it needs goes through host pointers) and libecb then runs on the system's HIP runtime, PyTorch not imported.
    if os.environ.get("ALNTOOLS_TORCH", "1") != "0" or "torch" in sys.modules:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s not found: build it with `python -m alntools_amd.build` "
                          "(the HIP path has no fallback)" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    lib.ecb_abi_version.restype = C.c_int
    if lib.ecb_abi_version() != ABI_VERSION and "ECB_LIB" not in os.environ:
        raise ImportError("%s has ABI %d, this binding is for ABI %d: rebuild it (python -m alntools_amd.build)"
                          % (LIB_PATH, lib.ecb_abi_version(), ABI_VERSION))
    _bind(lib, SIGNATURES)
    _lib = lib
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _dev_ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _side_stream(device, torch=None):
    """torch's current stream on CUDA device ``device`` where that is not the default stream, else None -- also where PyTorch is not
    imported or has not opened a GPU (no tensor can then be in flight).  libecb wants finished inputs and works on streams of its own
    (include/ecb.h); those order themselves behind torch's default stream, the legacy null stream, and behind no other: INTEGRATION.md,
    "Streams".  On the default stream this is two look-ups and nothing on the device."""
    torch = torch or sys.modules.get("torch")
    if torch is None or not torch.cuda.is_initialized():
        return None
    s = torch.cuda.current_stream(device)
    return None if s == torch.cuda.default_stream(device) else s


def _wait_side_stream(device, torch=None):
    """The host waits for what :func:`_side_stream` names, if it names a stream -> whether it did."""
    s = _side_stream(device, torch)
    if s is not None:
        s.synchronize()
    return s is not None


def _wait_device(device, torch=None):
    """The host waits for everything on CUDA device ``device``, libecb's own streams among it."""
    (torch or sys.modules["torch"]).cuda.synchronize(device)


def tile_tuples(read_id, locus, hapflag, out=None):
    """Three device arrays of ``n`` records -> one int32 tensor of whole tiles for :meth:`EcBuilder.push_device_tiled` (tile t = words
    ``[1536 t, 1536 t + 1536)`` = 512 read ids | 512 loci | 512 haplotype/flag words; the last tile's padding is zero)."""
    import torch
    n = read_id.numel()
    nt = (n + 511) // 512
    tiles = out if out is not None else torch.zeros(nt * 1536, dtype=torch.int32, device=read_id.device)
    v = tiles[:nt * 1536].view(nt, 3, 512)
    full = n // 512
    for k, src in enumerate((read_id, locus, hapflag)):
        src = src.view(torch.int32) if src.dtype != torch.int32 else src
        if full:
            v[:full, k, :] = src[:full * 512].view(full, 512)
        if n > full * 512:
            v[full, k, :n - full * 512] = src[full * 512:]
    return tiles


class _Numpy(object):
    """What a one-call wrapper asks of the arrays it was handed -- numpy arrays here: the host entry points, on the device the caller
    numbers.  :func:`_kind` picks this or :class:`_Torch` once per call; the wrapper then has one body for both."""
    tensors = False
    i32, i64, u32, u64, f64, u8 = np.int32, np.int64, np.uint32, np.uint64, np.float64, np.uint8
    ptr = staticmethod(_ptr)

    def __init__(self, device):
        self.device = device

    def entry(self, lib, name):
        return getattr(lib, name)

    def arr(self, a, dt):
        """``a`` as a contiguous array of type ``dt``, of this kind and on this device (None stays None)."""
        return None if a is None else np.ascontiguousarray(a, dtype=dt)

    def words(self, a, bits=32):
        """Unsigned words of ``bits`` bits as this kind carries them: a contiguous uint32 / uint64 array (None stays None)."""
        return self.arr(a, self.u32 if bits == 32 else self.u64)

    def flags(self, a):
        """uint8 0 / 1, flat, of anything truthy (None stays None)."""
        return None if a is None else np.ascontiguousarray(np.asarray(a) != 0, dtype=np.uint8).reshape(-1)

    def bytes(self, a):
        return np.frombuffer(a, dtype=np.uint8) if not isinstance(a, np.ndarray) else np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)

    def empty(self, shape, dt):
        return np.empty(shape, dtype=dt)

    def zeros(self, shape, dt):
        return np.zeros(shape, dtype=dt)

    def ready(self):
        """What every wrapper passes once, after its arrays are prepared and before its first call of the library: host arrays are
        always ready."""


class _Torch(_Numpy):
    """The same for tensors: the ``_device`` entry points, on the tensors' own device."""
    tensors = True
    ptr = staticmethod(_dev_ptr)

    def __init__(self, dev):
        import torch
        self.torch, self.dev, self.device = torch, dev, dev.index or 0
        self.i32, self.i64, self.f64, self.u8 = torch.int32, torch.int64, torch.float64, torch.uint8
        self.u32, self.u64 = torch.int32, torch.int64      # (torch computes with no unsigned words: the signed ones hold the same bytes)

    def entry(self, lib, name):
        return getattr(lib, name + "_device")

    def arr(self, a, dt):
        if a is None:
            return None
        return (a if isinstance(a, self.torch.Tensor) else self.torch.as_tensor(a)).to(self.dev, dt).contiguous()

    def words(self, a, bits=32):
        """... an int32 / int64 tensor holding the same bytes; what is no tensor yet gets there by a view of the unsigned numpy array."""
        if a is not None and not hasattr(a, "data_ptr"):
            a = np.ascontiguousarray(a, dtype=_Numpy.u32 if bits == 32 else _Numpy.u64).view(_Numpy.i32 if bits == 32 else _Numpy.i64)
        return self.arr(a, self.u32 if bits == 32 else self.u64)

    def flags(self, a):
        return None if a is None else self.torch.as_tensor(a).to(device=self.dev).ne(0).to(self.torch.uint8).contiguous().reshape(-1)

    def bytes(self, a):
        return a.contiguous().view(self.torch.uint8).reshape(-1)

    def empty(self, shape, dt):
        return self.torch.empty(shape, dtype=dt, device=self.dev)

    def zeros(self, shape, dt):
        """... and in place when it returns: off the default stream the host waits for the fill (the library would write first)."""
        z = self.torch.zeros(shape, dtype=dt, device=self.dev)
        _wait_side_stream(self.dev, self.torch)
        return z

    def ready(self):
        """... tensors may be in flight on torch's current stream -- the caller's kernels, the conversions of :meth:`arr` -- and the
        library waits for nothing of the caller's: off the default stream the host waits for that stream here.  (The other way round needs
        nothing: every entry point without a handle has waited for its own work when it returns.)"""
        _wait_side_stream(self.dev, self.torch)


_torch_kinds = {}


def _kind(first, device):
    """The kind of a call: of its first array, and for numpy arrays on the caller's ``device``."""
    if not hasattr(first, "data_ptr"):
        return _Numpy(device)
    k = _torch_kinds.get(first.device)
    if k is None:
        k = _torch_kinds[first.device] = _Torch(first.device)
    return k


def _matrices(k, mats):
    """CSR A and CSC N ``(indptr, indices, data) x 2`` as int32 of kind ``k`` -> (the six arrays, (E, nnz, S, nnz_n))."""
    a = [k.arr(x, k.i32) for x in mats]
    sizes = (len(a[0]) - 1, len(a[1]), len(a[3]) - 1, len(a[4]))
    if len(a[2]) != sizes[1] or len(a[5]) != sizes[3]:
        raise ValueError("indices and data differ in length")
    return a, sizes


def _check_tables(tabs, n_loci, n_haps, what):
    if any(t is not None and tuple(t.shape) != (n_haps, n_loci) for t in tabs):
        raise ValueError(what + " are [n_haps, n_loci]")


def _check_gene(gn, n_loci):
    if gn is not None and tuple(gn.shape) != (n_loci,):
        raise ValueError("gene is [n_loci]")


def csr_to_hapcsc(indptr, indices, data, n_loci, n_haps, nnz=None, device=0):
    """f-2 on device tensors (int32, CUDA): CSR(bitmask) -> (csc_indptr [H, T+1], csc_indices [total], nnz per haplotype).
    Haplotype h's row indices are ``csc_indices[starts[h]:starts[h+1]]`` (``bin_utils.ec2emase``'s per-haplotype CSC).
    One call when the row-index buffer sized for every non-zero carrying every haplotype (``nnz`` x H) stays below 1 GiB; beyond
    that (many haplotypes, sparse masks: up to 31 x what is needed) the library is asked for the count of set bits first.
    numpy arrays: :func:`csr_to_hapcsc_host`."""
    lib = load()
    k = _kind(indptr, device)
    p, fn = k.ptr, k.entry(lib, "ecb_csr_to_hapcsc")
    ip, ix, da = (k.arr(a, k.i32) for a in (indptr, indices, data))
    k.ready()
    head = (k.device, len(ip) - 1, n_loci, n_haps, p(ip), p(ix), p(da))
    room = (lambda n: ()) if k.tensors else (lambda n: (n,))      # what differs: only the host entry point is told csc_indices' room
    tot = C.c_uint64()
    cap = (len(ix) if nnz is None else int(nnz)) * n_haps
    if not k.tensors or cap >= (1 << 28):            # what differs: host arrays always get the count first (the exact size)
        _check(lib, fn(*head, None, None, *room(0), C.byref(tot)))
        cap = tot.value
    cptr = k.empty((n_haps, n_loci + 1), k.i32)
    cidx = k.empty(max(cap, 1), k.i32)
    _check(lib, fn(*head, p(cptr), p(cidx), *room(len(cidx)), C.byref(tot)))
    return cptr, cidx[:tot.value]


def csr_to_hapcsc_host(indptr, indices, data, n_loci, n_haps, device=0):
    """f-2 on HOST arrays (``ecb_csr_to_hapcsc``: the library holds the device buffers itself; no PyTorch involved):
    CSR(bitmask) -> (csc_indptr int32 [H, T+1], csc_indices int32 [total])."""
    return csr_to_hapcsc(indptr, indices, data, n_loci, n_haps, device=device)


def csr_to_hapcsc_values(indptr, indices, data, values, n_loci, n_haps, device=0):
    """:func:`csr_to_hapcsc` with a payload, on device tensors (``ecb_csr_to_hapcsc_values_device``): ``values`` float64, one per set bit of
    the masks in bit order (the non-zeros in storage order, the set bits of one lowest first: :func:`posterior`'s ``post``) ->
    (csc_indptr [H, T+1], csc_indices [total], csc_data float64 [total]); ``csc_data[k]`` is the value of the entry ``csc_indices[k]`` names.
    numpy arrays go through ``ecb_csr_to_hapcsc_values`` on ``device``."""
    lib = load()
    k = _kind(indptr, device)
    p, fn = k.ptr, k.entry(lib, "ecb_csr_to_hapcsc_values")
    ip, ix, da = (k.arr(a, k.i32) for a in (indptr, indices, data))
    va = k.arr(values, k.f64)
    k.ready()
    head = (k.device, len(ip) - 1, n_loci, n_haps, p(ip), p(ix), p(da))
    room = (lambda n: ()) if k.tensors else (lambda n: (n,))      # what differs: only the host entry point is told the outputs' room
    tot = C.c_uint64()
    _check(lib, fn(*head, None, None, None, None, *room(0), C.byref(tot)))
    if tot.value != len(va):
        raise ValueError("values holds %d entries, the matrix has %d set bits" % (len(va), tot.value))
    cptr = k.empty((n_haps, n_loci + 1), k.i32)
    cidx = k.empty(max(tot.value, 1), k.i32)
    cdat = k.empty(max(tot.value, 1), k.f64)
    _check(lib, fn(*head, p(va), p(cptr), p(cidx), p(cdat), *room(len(cidx)), C.byref(tot)))
    return cptr, cidx[:tot.value], cdat[:tot.value]


csr_to_hapcsc_values_host = csr_to_hapcsc_values       # (the name the host callers know)


def hapcsc_to_csr(csc_indptr, csc_indices, n_ecs, device=0):
    """f-2 inverse on device tensors: per-haplotype CSC -> CSR(bitmask) (``bin_utils.emase2ec``: A = sum 2^h M_h).  numpy arrays go
    through ``ecb_hapcsc_to_csr`` on ``device``; (indptr, indices, data), int32, of the same kind as the input."""
    lib = load()
    k = _kind(csc_indptr, device)
    p = k.ptr
    cptr, cidx = k.arr(csc_indptr, k.i32), k.arr(csc_indices, k.i32)
    k.ready()
    H, T1 = cptr.shape
    total = len(cidx)
    room = total if k.tensors else max(total, 1)     # what differs: tensors have always been sized exactly (an empty one's pointer is null)
    ip, ix, da = k.empty(n_ecs + 1, k.i32), k.empty(room, k.i32), k.empty(room, k.i32)
    nnz = C.c_uint64()
    _check(lib, k.entry(lib, "ecb_hapcsc_to_csr")(k.device, n_ecs, T1 - 1, H, p(cptr), p(cidx), total, p(ip), p(ix), p(da), C.byref(nnz)))
    return ip, ix[:nnz.value], da[:nnz.value]


hapcsc_to_csr_host = hapcsc_to_csr                     # (the name the host callers know)


def apply_mask(indptr, indices, data, mask, n_haps, device=0):
    """apply-genotypes on the GPU: CSR A (``.bin``'s bitmask values) with every value ANDed with ``mask[locus]``, the non-zeros that
    become 0 dropped, every row kept (``AlignmentPropertyMatrix.apply_genotypes``).  numpy arrays go through ``ecb_apply_mask`` (host
    arrays, no PyTorch), CUDA tensors through ``ecb_apply_mask_device`` (``device`` is then the tensors' own).  Returns (indptr, indices,
    data), int32, of the same kind as the input.  A malformed CSR or mask raises :class:`EcbError` (``ECB_ERR_CONTRACT``)."""
    lib = load()
    k = _kind(indptr, device)
    p = k.ptr
    ip, ix, da = (k.arr(a, k.i32) for a in (indptr, indices, data))
    mk = k.arr(mask, k.u32)
    k.ready()
    E, T, nnz = len(ip) - 1, len(mk), len(ix)
    if len(da) != nnz:
        raise ValueError("indices and data differ in length")
    oip, oix, oda = k.empty(E + 1, k.i32), k.empty(max(nnz, 1), k.i32), k.empty(max(nnz, 1), k.i32)
    kept = C.c_uint64()
    _check(lib, k.entry(lib, "ecb_apply_mask")(k.device, E, T, n_haps, nnz, p(ip), p(ix), p(da), p(mk), p(oip), p(oix), p(oda), C.byref(kept)))
    return oip, oix[:kept.value], oda[:kept.value]


def count_alignments(indptr, indices, data, n_loci, n_haps, indptr_n, indices_n, data_n, sample=None, device=0):
    """count-alignments on the GPU: the per-target read counts of CSR A (``.bin``'s bitmask values) weighted by CSC N -- the reference's
    ``count_alignments()``, ``count_unique_reads(ignore_haplotype=False)`` and ``count_unique_reads(ignore_haplotype=True)``
    (``AlignmentPropertyMatrix.py:429-448``).  ``sample``: None = every EC weighs the sum of its row of N, else the index of one column.
    numpy arrays go through ``ecb_count_alignments`` (host arrays, no PyTorch), CUDA tensors through ``ecb_count_alignments_device``
    (``device`` is then the tensors' own).  Returns ``(aln[H, T], uniq[H, T], locus_uniq[T])``, int64, of the same kind as the input.
    Malformed input or an unknown sample raises :class:`EcbError` (``ECB_ERR_CONTRACT``)."""
    lib = load()
    k = _kind(indptr, device)
    p = k.ptr
    s = -1 if sample is None else int(sample)
    (ip, ix, da, pn, xn, dn), (E, nnz, S, nnz_n) = _matrices(k, (indptr, indices, data, indptr_n, indices_n, data_n))
    k.ready()
    aln, uniq, lu = k.empty((n_haps, n_loci), k.i64), k.empty((n_haps, n_loci), k.i64), k.empty(n_loci, k.i64)
    _check(lib, k.entry(lib, "ecb_count_alignments")(k.device, E, n_loci, n_haps, nnz, p(ip), p(ix), p(da), S, nnz_n, p(pn), p(xn), p(dn), s,
                                                     p(aln), p(uniq), p(lu)))
    return aln, uniq, lu


def quantify(indptr, indices, data, n_loci, n_haps, indptr_n, indices_n, data_n, sample=None, scale=None, theta_in=None, max_iters=1000,
             tol=1e-6, device=0):
    """ecquant on the GPU: EM abundance estimates of CSR A (``.bin``'s bitmask values) weighted by CSC N -- the reference's ``multiply(axis=2)``,
    ``normalize_reads(axis=READ)``, ``sum(axis=READ)`` (``AlignmentPropertyMatrix.py:277-384``) iterated until the change of one step,
    summed over all entries, is at most ``tol`` times the reads that align, or ``max_iters`` steps have run.  ``sample`` as for
    :func:`count_alignments`; ``scale`` and ``theta_in``: float64 ``[H, T]`` or None (1 everywhere; the alignment counts).  numpy arrays go
    through ``ecb_quantify`` (host arrays, no PyTorch), CUDA tensors through ``ecb_quantify_device`` (``device`` is then the tensors' own).
    Returns ``(theta[H, T] float64, info)``, theta of the same kind as the input, ``info`` a dict with ``n_iter``, ``delta``, ``explained``
    and ``converged``.  Malformed input, an unknown sample or a NaN, infinite or negative entry of ``scale`` / ``theta_in`` raises
    :class:`EcbError` (``ECB_ERR_CONTRACT``)."""
    return _quantify((indptr, indices, data, indptr_n, indices_n, data_n), n_loci, n_haps, sample, scale, theta_in, max_iters, tol, device)


def _quantify(mats, n_loci, n_haps, sample, scale, theta_in, max_iters, tol, device, grouping=None):
    """:func:`quantify` and, with ``grouping = (gene, n_genes, model)``, :func:`quantify_model`: each through its own entry point."""
    lib = load()
    k = _kind(mats[0], device)
    p = k.ptr
    (ip, ix, da, pn, xn, dn), (E, nnz, S, nnz_n) = _matrices(k, mats)
    sc, th, gn = k.arr(scale, k.f64), k.arr(theta_in, k.f64), k.arr(grouping and grouping[0], k.i32)
    _check_gene(gn, n_loci)                          # (the genes before the tables here, after them per cell: the order each has always had)
    _check_tables((sc, th), n_loci, n_haps, "scale and theta_in")
    k.ready()
    s = -1 if sample is None else int(sample)
    it, dl, ex, cv = C.c_uint32(), C.c_double(), C.c_int64(), C.c_uint32()
    theta = k.empty((n_haps, n_loci), k.f64)
    fn = k.entry(lib, "ecb_quantify" + ("_model" if grouping else ""))
    model_args = (int(grouping[1]), p(gn), int(grouping[2])) if grouping else ()
    _check(lib, fn(k.device, E, n_loci, n_haps, nnz, p(ip), p(ix), p(da), S, nnz_n, p(pn), p(xn), p(dn), s, p(sc), p(th), int(max_iters), float(tol),
                   *model_args, p(theta), C.byref(it), C.byref(dl), C.byref(ex), C.byref(cv)))
    return theta, {"n_iter": it.value, "delta": dl.value, "explained": ex.value, "converged": bool(cv.value)}


def quantify_model(indptr, indices, data, n_loci, n_haps, indptr_n, indices_n, data_n, gene, n_genes, model, sample=None, scale=None,
                   theta_in=None, max_iters=1000, tol=1e-6, device=0):
    """ecquant with one of EMASE's models over a gene grouping (``ecb_quantify_model`` / ``ecb_quantify_model_device``): :func:`quantify`
    with ``gene`` (int32 ``[T]``, ``gene[t]`` in ``[0, n_genes)``) and ``model`` -- 1 gene -> allele -> isoform, 2 gene -> isoform -> allele,
    3 gene -> isoform x allele, 4 the flat step of :func:`quantify`, whose bytes it then returns.  Everything else, the kinds of the arrays
    and the result as for :func:`quantify`.  A gene id outside ``[0, n_genes)`` raises :class:`EcbError` (``ECB_ERR_CONTRACT``), a model
    outside 1..4 ``ECB_ERR_ARG``."""
    return _quantify((indptr, indices, data, indptr_n, indices_n, data_n), n_loci, n_haps, sample, scale, theta_in, max_iters, tol, device,
                     grouping=(gene, n_genes, model))


def posterior(indptr, indices, data, n_loci, n_haps, theta, scale=None, gene=None, n_genes=0, model=4, device=0):
    """The posterior probability of every alignment at ``theta`` (``ecb_posterior`` / ``ecb_posterior_device``): one value per set bit of CSR
    A (``.bin``'s bitmask values) -- model 4: ``phi[h, t] / d[e]`` with ``phi = theta * scale``; models 1-3: the factor product of
    :func:`quantify_model` over ``gene`` -- so that the sum over rows of ``w[e]`` times it is one step of :func:`quantify` /
    :func:`quantify_model` from ``theta``.  ``theta``, ``scale``: float64 ``[H, T]`` (``scale`` may be None); ``gene`` may be None for model 4.
    numpy arrays go through the host entry point, CUDA tensors through the device one (``device`` is then the tensors' own).  Returns
    ``(post float64 [n_bits], bit_ptr int64 [nnz + 1], row_mass float64 [E])`` of the same kind as the input: ``post`` in bit order -- the
    non-zeros in storage order, the set bits of one lowest first, non-zero i owning ``post[bit_ptr[i]:bit_ptr[i + 1]]`` -- and ``row_mass[e]``
    the row's normalizing sum, 0 for a row nothing explains (all of it is then 0).  A NaN, infinite or negative entry of ``theta`` or
    ``scale``, a gene id outside ``[0, n_genes)`` or a malformed A raises :class:`EcbError` (``ECB_ERR_CONTRACT``)."""
    lib = load()
    k = _kind(indptr, device)
    p = k.ptr
    ip, ix, da = (k.arr(a, k.i32) for a in (indptr, indices, data))
    sc, th, gn = k.arr(scale, k.f64), k.arr(theta, k.f64), k.arr(gene, k.i32)
    E, nnz = len(ip) - 1, len(ix)
    k.ready()
    # what differs: how the set bits are counted -- host masks here, device masks by the conversion's count-only call (one pass over the
    # masks it is told of), and only over a CSR it can walk
    n_bits = 0
    if not k.tensors:
        n_bits = int(np.unpackbits(da.view(np.uint8)).sum())
    elif E > 0 and nnz and len(da) == nnz and int(ip[-1]) == nnz:
        tot = C.c_uint64()
        _check(lib, lib.ecb_csr_to_hapcsc_device(k.device, E, n_loci, n_haps, p(ip), p(ix), p(da), None, None, C.byref(tot)))
        n_bits = tot.value
    if len(da) != nnz:
        raise ValueError("indices and data differ in length")
    if th is None:
        raise ValueError("theta and scale are [n_haps, n_loci]")
    _check_tables((sc, th), n_loci, n_haps, "theta and scale")
    _check_gene(gn, n_loci)
    post, bit_ptr, row_mass = k.zeros(n_bits, k.f64), k.zeros(nnz + 1, k.i64), k.zeros(E, k.f64)
    _check(lib, k.entry(lib, "ecb_posterior")(k.device, E, n_loci, n_haps, nnz, p(ip), p(ix), p(da), p(sc), p(th), int(n_genes), p(gn), int(model),
                                              n_bits, p(post) if n_bits else None, p(bit_ptr), p(row_mass)))
    return post, bit_ptr, row_mass


def _cell_keep(k, cell_keep, n_samples):
    keep = k.flags(cell_keep)
    if keep is not None and len(keep) != n_samples:
        raise ValueError("cell_keep is [n_samples]")
    return keep


def cell_support(indptr, indices, data, n_loci, n_haps, indptr_n, indices_n, data_n, cell_keep=None, device=0, count_only=False):
    """The targets detected per cell (``ecb_cell_support`` / ``ecb_cell_support_device``): for every column c of CSC N, the loci at which an EC
    the cell counts (> 0) holds a mask other than 0, ascending.  ``cell_keep``: ``[n_samples]``, non-zero = this cell, None = every cell.
    numpy arrays go through the host entry point, CUDA tensors through the device one.  Returns ``(cell_ptr int64 [S + 1], slot_locus int32
    [n_slots])`` of the same kind as the input: cell c owns ``slot_locus[cell_ptr[c]:cell_ptr[c + 1]]``.  ``count_only``: one pass instead of
    two, ``slot_locus`` is then None."""
    lib = load()
    k = _kind(indptr, device)
    mats, sizes = _matrices(k, (indptr, indices, data, indptr_n, indices_n, data_n))
    keep = _cell_keep(k, cell_keep, sizes[2])
    k.ready()
    return _cell_support(lib, k, mats, sizes, keep, n_loci, n_haps, count_only)


def _cell_support(lib, k, mats, sizes, keep, n_loci, n_haps, count_only):
    """:func:`cell_support` on arrays of kind ``k`` that are prepared and ready (:func:`_quantify_cells` sizes its support here)."""
    p, fn = k.ptr, k.entry(lib, "ecb_cell_support")
    (ip, ix, da, pn, xn, dn), (E, nnz, S, nnz_n) = mats, sizes
    ns = C.c_uint64()
    head = (k.device, E, n_loci, n_haps, nnz, p(ip), p(ix), p(da), S, nnz_n, p(pn), p(xn), p(dn), p(keep))
    cell_ptr = k.empty(S + 1, k.i64)
    _check(lib, fn(*(head + (p(cell_ptr), None, 0, C.byref(ns)))))       # (the sizes first ...
    if count_only:
        return cell_ptr, None
    slot_locus = k.empty(ns.value, k.i32)
    if ns.value:
        _check(lib, fn(*(head + (p(cell_ptr), p(slot_locus), ns.value, C.byref(ns)))))      # ... then the loci, into an array that fits)
    return cell_ptr, slot_locus


def quantify_cells(indptr, indices, data, n_loci, n_haps, indptr_n, indices_n, data_n, cell_keep=None, scale=None, theta_in=None, max_iters=1000,
                   tol=1e-6, budget_bytes=0, device=0, n_slots=None):
    """ecquant per cell on the GPU (``ecb_quantify_cells`` / ``ecb_quantify_cells_device``): one EM of :func:`quantify` for every column of N
    that ``cell_keep`` names (None: all), each over its own support and stopping at its own step, all iterated by the same launches.
    ``scale`` and ``theta_in``: float64 ``[H, T]`` or None, shared by every cell.  ``budget_bytes``: the device memory a batch of cells aims at
    (0: half of what is free); the result does not depend on it.  numpy arrays go through the host entry point, CUDA tensors through the
    device one.  Returns ``(cell_ptr int64 [S + 1], slot_locus int32 [n_slots], theta float64 [n_slots, H], info)`` of the same kind as the
    input; ``info`` is a dict of per-cell arrays ``n_iter`` (uint32; int64 for tensors), ``delta`` (float64), ``explained`` (int64) and ``converged`` (bool).
    The support is sized by :func:`cell_support` first, unless the caller passes the ``n_slots`` it learned there."""
    return _quantify_cells((indptr, indices, data, indptr_n, indices_n, data_n), n_loci, n_haps, cell_keep, scale, theta_in, max_iters, tol, budget_bytes,
                           device, n_slots)


def _quantify_cells(mats, n_loci, n_haps, cell_keep, scale, theta_in, max_iters, tol, budget_bytes, device, n_slots, grouping=None):
    """:func:`quantify_cells` and, with ``grouping = (gene, n_genes, model)``, :func:`quantify_cells_model`: each through its own entry point."""
    lib = load()
    k = _kind(mats[0], device)
    p = k.ptr
    (ip, ix, da, pn, xn, dn), (E, nnz, S, nnz_n) = _matrices(k, mats)
    keep = _cell_keep(k, cell_keep, S)
    sc, th, gn = k.arr(scale, k.f64), k.arr(theta_in, k.f64), k.arr(grouping and grouping[0], k.i32)
    _check_tables((sc, th), n_loci, n_haps, "scale and theta_in")
    _check_gene(gn, n_loci)
    k.ready()
    if n_slots is None:
        n_slots = int(_cell_support(lib, k, (ip, ix, da, pn, xn, dn), (E, nnz, S, nnz_n), keep, n_loci, n_haps, True)[0][-1])
    fn = k.entry(lib, "ecb_quantify_cells" + ("_model" if grouping else ""))
    model_args = (int(grouping[1]), p(gn), int(grouping[2])) if grouping else ()
    cell_ptr, slot_locus, theta = k.empty(S + 1, k.i64), k.empty(n_slots, k.i32), k.empty((n_slots, n_haps), k.f64)
    it, dl, ex, cv = k.empty(S, k.u32), k.empty(S, k.f64), k.empty(S, k.i64), k.empty(S, k.u8)
    _check(lib, fn(k.device, E, n_loci, n_haps, nnz, p(ip), p(ix), p(da), S, nnz_n, p(pn), p(xn), p(dn), p(keep), p(sc), p(th), int(max_iters),
                   float(tol), int(budget_bytes), *model_args, n_slots, p(cell_ptr), p(slot_locus), p(theta), p(it), p(dl), p(ex), p(cv)))
    if k.tensors:                                    # what differs: the uint32 the library wrote, in a type torch computes with
        it = it.to(k.i64).bitwise_and(0xFFFFFFFF)
    return cell_ptr, slot_locus, theta, {"n_iter": it, "delta": dl, "explained": ex, "converged": cv != 0}


def quantify_cells_model(indptr, indices, data, n_loci, n_haps, indptr_n, indices_n, data_n, gene, n_genes, model, cell_keep=None, scale=None,
                         theta_in=None, max_iters=1000, tol=1e-6, budget_bytes=0, device=0, n_slots=None):
    """ecquant per cell with one of EMASE's models over a gene grouping (``ecb_quantify_cells_model`` / ``ecb_quantify_cells_model_device``):
    :func:`quantify_cells` with ``gene`` (int32 ``[T]``, ``gene[t]`` in ``[0, n_genes)``) and ``model`` as :func:`quantify_model` numbers them;
    model 4 returns the bytes of :func:`quantify_cells`.  Every cell is a problem of its own: the sums over a gene run over the cell's support
    only, so a member the cell does not touch contributes nothing, whatever ``theta_in`` holds there.  Everything else, the kinds of the
    arrays and the result as for :func:`quantify_cells`.  A gene id outside ``[0, n_genes)`` raises :class:`EcbError` (``ECB_ERR_CONTRACT``),
    a model outside 1..4 ``ECB_ERR_ARG``."""
    return _quantify_cells((indptr, indices, data, indptr_n, indices_n, data_n), n_loci, n_haps, cell_keep, scale, theta_in, max_iters, tol, budget_bytes,
                           device, n_slots, grouping=(gene, n_genes, model))


def combine(parts, n_loci, n_haps, n_samples, device=0):
    """ecmerge on the GPU: several ``.bin`` files' A and N as one (``ecb_combine``).  ``parts``: one dict per input with ``indptrA,
    indicesA, dataA, indptrN, indicesN, dataN`` (CSR A and CSC N as the file stores them), ``n_loci`` (the file's targets),
    ``target_map`` (the file's column -> merged column, or None: the same numbering) and ``sample_map`` (the file's sample -> output
    sample).  Rows with equal keys become one EC, numbered by first appearance; counts add per (EC, sample), zero sums are dropped.
    numpy arrays go through ``ecb_combine`` (host arrays, no PyTorch), CUDA tensors through ``ecb_combine_device`` (``device`` is then
    the tensors' own).  Returns (indptrA, indicesA, dataA, indptrN, indicesN, dataN), int32, of the same kind as the input.  Malformed
    input raises :class:`EcbError` (``ECB_ERR_CONTRACT``), sizes beyond the format's limits ``ECB_ERR_LIMIT``."""
    lib = load()
    k = _kind(parts[0]["indptrA"] if parts else None, device)
    held, cp = [], (CombinePart * max(len(parts), 1))()
    R = NP = NZ = 0
    for i, part in enumerate(parts):
        a = [k.arr(part[n], k.i32) for n in ("indptrA", "indicesA", "dataA", "indptrN", "indicesN", "dataN")]
        a += [k.arr(part.get(n), k.i32) for n in ("target_map", "sample_map")]     # (a map's values are below 2^31: int32 and uint32 are the same bytes)
        held += a
        E, S = len(a[0]) - 1, len(a[3]) - 1
        if len(a[1]) != len(a[2]) or len(a[4]) != len(a[5]):
            raise ValueError("part %d: indices and data differ in length" % i)
        c = cp[i]
        c.struct_size, c.n_ecs, c.n_samples, c.n_loci = C.sizeof(CombinePart), E, S, int(part["n_loci"])
        c.nnz_a, c.nnz_n = len(a[1]), len(a[4])
        for n, x in zip(("indptr_a", "indices_a", "data_a", "indptr_n", "indices_n", "data_n", "target_map", "sample_map"), a):
            setattr(c, n, None if x is None else k.ptr(x).value)
        R, NP, NZ = R + E, NP + len(a[1]), NZ + len(a[4])
    k.ready()
    out = [k.empty(max(n, 1), k.i32) for n in (R + 1, NP, NP, n_samples + 1, NZ, NZ)]
    sizes = (C.c_uint64 * 3)()
    _check(lib, k.entry(lib, "ecb_combine")(k.device, len(parts), cp, n_loci, n_haps, n_samples, *[k.ptr(o) for o in out], sizes))
    E, nnz_a, nnz_n = (int(x) for x in sizes)
    return out[0][:E + 1], out[1][:nnz_a], out[2][:nnz_a], out[3], out[4][:nnz_n], out[5][:nnz_n]


def bundle(indptrA, indicesA, dataA, indptrN, indicesN, dataN, n_loci, n_haps, n_groups, map_ptr, map_idx, device=0):
    """ecbundle on the GPU: the columns of one ``.bin``'s CSR A collapsed into groups and its rows folded back into ECs (``ecb_bundle``).
    ``map_ptr`` (``n_loci + 1``) and ``map_idx`` are the group map as a CSR over the loci: the group ids of every locus, strictly
    ascending, below ``n_groups``; a locus may have one, none or several.  The mask at (row, group) is the OR of the row's masks over the
    group's loci; rows with equal (group, mask) sets become one EC, numbered by first appearance; counts add per (EC, sample), zero sums
    are dropped.  numpy arrays go through ``ecb_bundle`` (host arrays, no PyTorch), CUDA tensors through ``ecb_bundle_device``
    (``device`` is then the tensors' own).  Returns (indptrA, indicesA, dataA, indptrN, indicesN, dataN), int32, of the same kind as the
    input.  Malformed input or a malformed map raises :class:`EcbError` (``ECB_ERR_CONTRACT``), sizes beyond the limits ``ECB_ERR_LIMIT``."""
    lib = load()
    k = _kind(indptrA, device)
    p = k.ptr
    (ipa, ixa, daa, ipn, ixn, dan), (E, nnz, S, nnz_n) = _matrices(k, (indptrA, indicesA, dataA, indptrN, indicesN, dataN))
    mp, mi = k.arr(map_ptr, k.i32), k.arr(map_idx, k.i32)             # (a map's values are below 2^31: int32 and uint32 are the same bytes)
    if len(mp) != n_loci + 1:
        raise ValueError("map_ptr has %d entries for %d loci" % (len(mp), n_loci))
    # room for A: the (row, group) pairs before the fold -- one per non-zero and group of its locus, where the map and the columns can be
    # indexed at all (otherwise the library refuses before it writes) -- and never more than a full matrix
    cap = 0
    if nnz and len(mp) > 1:                          # what differs: how each kind spells a clamped difference and a clamped index
        per = (mp[1:] - mp[:-1]).clamp(min=0) if k.tensors else np.maximum(np.diff(mp.astype(np.int64)), 0)
        cols = ixa.long().clamp(0, n_loci - 1) if k.tensors else np.clip(ixa, 0, n_loci - 1)
        cap = min(int(per[cols].sum()), E * n_groups, (1 << 31) - 1)
    k.ready()
    out = [k.empty(max(n, 1), k.i32) for n in (E + 1, cap, cap, S + 1, nnz_n, nnz_n)]
    sizes = (C.c_uint64 * 3)()
    _check(lib, k.entry(lib, "ecb_bundle")(k.device, E, n_loci, n_haps, S, n_groups, nnz, p(ipa), p(ixa), p(daa), nnz_n, p(ipn), p(ixn), p(dan),
                                           len(mi), p(mp), p(mi), cap, *([p(o) for o in out] + [sizes])))
    E2, nnz_a, nnz_n2 = (int(x) for x in sizes)
    return out[0][:E2 + 1], out[1][:nnz_a], out[2][:nnz_a], out[3], out[4][:nnz_n2], out[5][:nnz_n2]


def select(indptrA, indicesA, dataA, indptrN, indicesN, dataN, n_loci, n_haps, row_class=None, sample_keep=None, min_count=None, device=0):
    """ecselect on the GPU: the reads of one class and the samples that still count enough of them, pulled out of one ``.bin``'s CSR A and
    CSC N (``ecb_select``).  ``row_class``: None or ``"all"`` (every row), ``"unique"`` (one set bit in the whole row), ``"locus-unique"`` (one
    non-zero with a mask other than 0) or ``"multi"`` (two or more), or its number 0 .. 3.  ``sample_keep``: per sample whether it is named
    (None: all are).  ``min_count``: None, or the threshold a named sample's total over the rows in class must reach (``max(min_count, 1)``,
    the reference's rule).  Entries of N stay when their row is in class, their sample stays and their count is above 0; rows stay when an
    entry of theirs does, in order, renumbered from 0.  numpy arrays go through ``ecb_select`` (host arrays, no PyTorch), CUDA tensors
    through ``ecb_select_device`` (``device`` is then the tensors' own).  Returns ``((indptrA, indicesA, dataA, indptrN, indicesN, dataN),
    kept)``: int32 arrays of the same kind as the input, and a bool array, per sample of the input whether it stayed.  A result without a
    sample or without a row is returned as it is.  Malformed input raises :class:`EcbError` (``ECB_ERR_CONTRACT``)."""
    lib = load()
    k = _kind(indptrA, device)
    p = k.ptr
    rc = ROW_CLASSES[row_class] if row_class is None or isinstance(row_class, str) else int(row_class)
    mc = -1 if min_count is None else max(int(min_count), 0)
    (ipa, ixa, daa, ipn, ixn, dan), (E, nnz, S, nnz_n) = _matrices(k, (indptrA, indicesA, dataA, indptrN, indicesN, dataN))
    sk = k.flags(sample_keep)
    if sk is not None and len(sk) != S:
        raise ValueError("sample_keep has %d entries for %d samples" % (len(sk), S))
    k.ready()
    out = [k.empty(max(n, 1), k.i32) for n in (E + 1, nnz, nnz, S + 1, nnz_n, nnz_n)]
    kept = k.empty(max(S, 1), k.u8)
    sizes = (C.c_uint64 * 4)()
    _check(lib, k.entry(lib, "ecb_select")(k.device, E, n_loci, n_haps, S, nnz, p(ipa), p(ixa), p(daa), nnz_n, p(ipn), p(ixn), p(dan), rc, p(sk), mc,
                                           *([p(o) for o in out] + [p(kept), sizes])))
    E2, nnz_a, S2, nnz_n2 = (int(x) for x in sizes)
    return (out[0][:E2 + 1], out[1][:nnz_a], out[2][:nnz_a], out[3][:S2 + 1], out[4][:nnz_n2], out[5][:nnz_n2]), kept[:S] != 0


#: ``ecb_salmon_ecs``'s reason codes (include/ecb.h)
SALMON_REASONS = {1: "a byte other than a digit, tab or line end", 2: "an empty field", 3: "a value of 2^31 or more",
                  4: "fewer than 2 fields", 5: "k differs from the number of target ids", 6: "a target id at or beyond the number of targets",
                  7: "a target id repeated within the line", 8: "the number of EC lines differs from the header's"}


class SalmonFormatError(OffenderError):
    """``ecb_salmon_ecs`` refused the EC section: ``line`` is the lowest offending EC line (0-based), ``reason`` its code."""

    def __init__(self, code, msg, line, reason):
        OffenderError.__init__(self, code, msg, "EC line", line)
        self.reason = reason

    line = property(lambda self: self.index)


_SALMON_REFUSAL = re.compile(r"EC line (\d+): .* \(reason (\d+)\)$")


def salmon_ecs(text, n_ecs, target_col, target_hap, n_loci, n_haps, device=0):
    """salmon2ec on the GPU: CSR A and N of the EC section of a salmon ``eq_classes.txt`` (the bytes after the target names;
    ``ecb_salmon_ecs``).  ``target_col[t]`` / ``target_hap[t]``: the column and haplotype of salmon target t.  A bytes-like ``text``
    goes through ``ecb_salmon_ecs`` (host arrays, no PyTorch), a CUDA uint8 tensor through ``ecb_salmon_ecs_device`` (with the
    other arrays moved to its device).  Returns (indptrA, indicesA, dataA, indicesN, dataN), int32, N's being the ECs with a non-zero
    count and their counts.  A malformed text raises :class:`SalmonFormatError` with the lowest offending line; sizes beyond the
    limits raise :class:`EcbError` (``ECB_ERR_LIMIT``)."""
    lib = load()
    k = _kind(text, device)
    p = k.ptr
    t = k.bytes(text)
    cap = max(int((t == 9).sum()) - n_ecs, 0)          # (target ids = tabs - E in a well-formed text: the non-zeros' bound)
    if k.tensors:                                    # what differs: a tensor is made of the ids as int64 (torch takes no uint32 array everywhere)
        target_col, target_hap = (np.asarray(a, dtype=np.int64) for a in (target_col, target_hap))
    tc, th = k.arr(target_col, k.u32), k.arr(target_hap, k.u32)
    if not k.tensors and len(tc) != len(th):         # what differs: only the host arrays have ever been compared
        raise ValueError("target_col and target_hap differ in length")
    k.ready()
    out = [k.empty(n, k.i32) for n in (n_ecs + 1, max(cap, 1), max(cap, 1), max(n_ecs, 1), max(n_ecs, 1))]
    sizes = (C.c_uint64 * 2)()
    _check_offender(lib, k.entry(lib, "ecb_salmon_ecs")(k.device, p(t), len(t), n_ecs, len(tc), p(tc), p(th), n_loci, n_haps, cap, *[p(o) for o in out], sizes),
                    _SALMON_REFUSAL, SalmonFormatError)
    nnz, nnz_n = int(sizes[0]), int(sizes[1])
    return out[0], out[1][:nnz], out[2][:nnz], out[3][:nnz_n], out[4][:nnz_n]


class EcBuilder(object):
    """One handle = one GPU.  Push record tuples, finalize, read back CSR A and N."""

    def __init__(self, n_loci, n_haplotypes, device=0, track_ranges=False, ec_capacity=0,
                 arena_capacity=0, max_batch_records=0, multisample=False, verify=False):
        self._lib = load()
        self._h = C.c_void_p()
        flags = (F_RANGES if track_ranges else 0) | (F_MULTISAMPLE if multisample else 0) | (F_VERIFY if verify else 0)
        self.multisample = multisample
        cfg = Config(C.sizeof(Config), device, n_loci, n_haplotypes, flags, 0, ec_capacity,
                     arena_capacity, max_batch_records)
        _check(self._lib, self._lib.ecb_create(C.byref(cfg), C.byref(self._h)))
        self.n_loci, self.n_haplotypes, self.track_ranges = n_loci, n_haplotypes, track_ranges
        self.device = device
        self.sizes = None

    # -- plumbing ------------------------------------------------------------
    def _chk(self, rc):
        _check(self._lib, rc, self._h)

    def _device_call(self, *calls):
        """Every ``*_device`` method's way into the library: ``calls`` = ``(function, argument after the handle, ...)``, made in order.
        The tensors behind the pointers may be in flight on torch's current stream, and the handle works on a stream of its own that
        waits for nothing of the caller's and that some entry points do not wait for either (include/ecb.h: "no wait").  On the default
        stream both orderings are given (:func:`_side_stream`); off it the host waits for the caller's stream before the first call and
        for the device after the last, so that what the caller queues next finds the library's reads and writes done."""
        side = _wait_side_stream(self.device)
        try:
            for c in calls:
                self._chk(c[0](self._h, *c[1:]))
        finally:
            if side:
                _wait_device(self.device)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.ecb_destroy(self._h)
            self._h = None          # (not C.c_void_p(): at interpreter shutdown the ctypes module may already be gone)

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def reset(self):
        """Forget all input and results; allocations (table, arena, staging) are kept."""
        self._chk(self._lib.ecb_reset(self._h))
        self.sizes = None

    # -- input ---------------------------------------------------------------
    def push(self, read_id, locus, hapflag, pos=None):
        """Host (numpy) tuple streams; a read may straddle calls."""
        rid = np.ascontiguousarray(read_id, dtype=np.uint32)
        loc = np.ascontiguousarray(locus, dtype=np.uint32)
        hf = np.ascontiguousarray(hapflag, dtype=np.uint32)
        ps = None if pos is None else np.ascontiguousarray(pos, dtype=np.int32)
        if not (len(rid) == len(loc) == len(hf)) or (ps is not None and len(ps) != len(rid)):
            raise ValueError("tuple streams differ in length")
        self._chk(self._lib.ecb_push(self._h, _ptr(rid), _ptr(loc), _ptr(hf), _ptr(ps), len(rid)))

    def push_device(self, read_id, locus, hapflag, pos=None):
        """torch tensors already in HBM (int32/uint32 bit patterns); whole reads per call."""
        n = read_id.numel()
        for t in (read_id, locus, hapflag) + ((pos,) if pos is not None else ()):
            if not t.is_cuda or not t.is_contiguous() or t.element_size() != 4 or t.numel() != n:
                raise ValueError("device tuple streams must be contiguous 4-byte CUDA tensors of equal length")
        self._device_call((self._lib.ecb_push_device, _dev_ptr(read_id), _dev_ptr(locus), _dev_ptr(hapflag), _dev_ptr(pos), n))

    def push_device_tiled(self, tiles, n):
        """``n`` records in ONE int32 CUDA tensor of whole tiles (``ecb_push_device_tiled``: 512 read ids | 512 loci | 512 haplotype/flag
        words per tile, ``ceil(n / 512) * 1536`` words); whole reads per call.  :func:`tile_tuples` lays three arrays out this way."""
        if not tiles.is_cuda or not tiles.is_contiguous() or tiles.element_size() != 4 or tiles.numel() < (n + 511) // 512 * 1536:
            raise ValueError("tiles: a contiguous 4-byte CUDA tensor of ceil(n / 512) * 1536 words")
        self._device_call((self._lib.ecb_push_device_tiled, _dev_ptr(tiles), n))

    def verify_device_tiled(self, tiles, n):
        bad, skipped = C.c_uint64(), C.c_uint64()
        self._device_call((self._lib.ecb_verify_device_tiled, _dev_ptr(tiles), n, C.byref(bad), C.byref(skipped)))
        return bad.value, skipped.value

    def hint_reads(self, max_reads):
        """The stream holds at most ``max_reads`` reads: ``push_device`` then waits for the device once per call, not twice
        (``ecb_hint_reads``; running past the bound is a contract error; 0 takes the bound back)."""
        self._chk(self._lib.ecb_hint_reads(self._h, int(max_reads)))

    def verify_device(self, read_id, locus, hapflag):
        """Independent exactness pass over the device-resident stream that was pushed: -> (reads whose target set differs
        from their EC's stored key, reads that took the long-read compare)."""
        bad, skipped = C.c_uint64(), C.c_uint64()
        self._device_call((self._lib.ecb_verify_device, _dev_ptr(read_id), _dev_ptr(locus), _dev_ptr(hapflag), read_id.numel(), C.byref(bad),
                           C.byref(skipped)))
        return bad.value, skipped.value

    def push_cells(self, meta, first_read):
        """Multisample: ``cell | file << 22`` of reads ``[first_read, first_read + len(meta))``."""
        m = np.ascontiguousarray(meta, dtype=np.uint32)
        self._chk(self._lib.ecb_push_cells(self._h, _ptr(m), first_read, len(m)))

    def push_cells_device(self, meta, first_read):
        """The same from an int32 CUDA tensor (kept alive by the caller until ``finalize``)."""
        self._device_call((self._lib.ecb_push_cells_device, _dev_ptr(meta), first_read, meta.numel()))

    def ms_filter_sizes(self, n_cells, minimum_count):
        """``ecb_ms_filter`` alone: the result stays on the device (``ms_filter`` also copies it to the host) -> its sizes."""
        m = MsSizes()
        self._chk(self._lib.ecb_ms_filter(self._h, n_cells, minimum_count, C.byref(m)))
        return {k: int(getattr(m, k)) for k, _ in MsSizes._fields_}

    # -- results -------------------------------------------------------------
    def finalize(self):
        s = Sizes()
        self._chk(self._lib.ecb_finalize(self._h, C.byref(s)))
        self.sizes = {k: int(getattr(s, k)) for k, _ in Sizes._fields_}
        return self.sizes

    def export(self):
        """-> dict of int32 numpy arrays: indptrA, indicesA, dataA, indptrN, indicesN, dataN."""
        s = self.sizes or self.finalize()
        E, nnz, S, nnzn = s["n_ecs"], s["nnz_a"], s["n_samples"], s["nnz_n"]
        out = dict(indptrA=np.empty(E + 1, np.int32), indicesA=np.empty(nnz, np.int32),
                   dataA=np.empty(nnz, np.int32))
        if self.multisample:
            self._chk(self._lib.ecb_export(self._h, _ptr(out["indptrA"]), _ptr(out["indicesA"]), _ptr(out["dataA"]),
                                           None, None, None))
            return out
        out.update(indptrN=np.empty(S + 1, np.int32), indicesN=np.empty(nnzn, np.int32), dataN=np.empty(nnzn, np.int32))
        self._chk(self._lib.ecb_export(self._h, *[_ptr(out[k]) for k in
                                                  ("indptrA", "indicesA", "dataA", "indptrN", "indicesN", "dataN")]))
        return out

    def export_pairs(self):
        """Multisample: distinct (EC, cell, file) triples -> dict(ec, cell, file, count, first), sorted by (ec, cell, file)."""
        s = self.sizes or self.finalize()
        n = s["nnz_n"]
        ec, meta, cnt, first = (np.empty(n, np.uint32) for _ in range(4))
        self._chk(self._lib.ecb_export_pairs(self._h, _ptr(ec), _ptr(meta), _ptr(cnt), _ptr(first)))
        return dict(ec=ec.astype(np.int64), cell=(meta & ((1 << 22) - 1)).astype(np.int64), file=(meta >> 22).astype(np.int64),
                    count=cnt.astype(np.int64), first=first.astype(np.int64))

    def ms_filter(self, n_cells, minimum_count):
        """Multisample, after finalize: cell order, minimum-count filter, EC re-rank, CSC N and the surviving rows of A, on
        the device (``bam_utils_multisample.py:596-636, 737-791``) -> dict(kept_cells [cell ids in sample order], indptrA,
        indicesA, dataA, indptrN, indicesN, dataN, n_cells_seen)."""
        m = MsSizes()
        self._chk(self._lib.ecb_ms_filter(self._h, n_cells, minimum_count, C.byref(m)))
        S, E2, nnza, nnzn = int(m.n_cells_kept), int(m.n_ecs_kept), int(m.nnz_a), int(m.nnz_n)
        out = dict(kept_cells=np.empty(S, np.uint32), indptrA=np.empty(E2 + 1, np.int32), indicesA=np.empty(nnza, np.int32),
                   dataA=np.empty(nnza, np.int32), indptrN=np.empty(S + 1, np.int32), indicesN=np.empty(nnzn, np.int32),
                   dataN=np.empty(nnzn, np.int32))
        self._chk(self._lib.ecb_ms_export(self._h, *[_ptr(out[k]) for k in
                                                     ("kept_cells", "indptrA", "indicesA", "dataA", "indptrN", "indicesN", "dataN")]))
        out["n_cells_seen"] = int(m.n_cells_seen)
        return out

    def export_ranges(self):
        out = np.empty((self.n_loci, self.n_haplotypes), np.int64)
        self._chk(self._lib.ecb_export_ranges(self._h, _ptr(out)))
        return out

    def export_range_minmax(self):
        mn = np.empty((self.n_loci, self.n_haplotypes), np.int32)
        mx = np.empty((self.n_loci, self.n_haplotypes), np.int32)
        self._chk(self._lib.ecb_export_range_minmax(self._h, _ptr(mn), _ptr(mx)))
        return mn, mx

    def export_read_ec(self):
        s = self.sizes or self.finalize()
        out = np.empty(s["n_reads"], np.int32)
        self._chk(self._lib.ecb_export_read_ec(self._h, _ptr(out)))
        return out

    # -- multi-GPU -----------------------------------------------------------
    def table_sizes(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._chk(self._lib.ecb_table_sizes(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def table_export_device(self, entries, pairs, read_base):
        self._device_call((self._lib.ecb_table_export_device, _dev_ptr(entries), _dev_ptr(pairs), read_base))

    def table_merge_device(self, entries, n_entries, pairs, n_pairs):
        self._device_call((self._lib.ecb_table_merge_device, _dev_ptr(entries), n_entries, _dev_ptr(pairs), n_pairs))

    def table_export_parts_device(self, entries, pairs, read_base, n_parts):
        """Export grouped into ``n_parts`` key ranges -> (entry_offsets, pair_offsets), lists of n_parts + 1."""
        eo, po = (C.c_uint64 * (n_parts + 1))(), (C.c_uint64 * (n_parts + 1))()
        self._device_call((self._lib.ecb_table_export_parts_device, _dev_ptr(entries), _dev_ptr(pairs), read_base, n_parts, eo, po))
        return list(eo), list(po)

    def _batch(self, fn, tables):
        """``tables``: list of (entries tensor, n_entries, pairs tensor, n_pairs)."""
        n = len(tables)
        pe, ne = (C.c_void_p * n)(*[t[0].data_ptr() for t in tables]), (C.c_uint64 * n)(*[t[1] for t in tables])
        pp, npr = (C.c_void_p * n)(*[t[2].data_ptr() for t in tables]), (C.c_uint64 * n)(*[t[3] for t in tables])
        self._device_call((fn, n, pe, ne, pp, npr))

    def table_merge_batch_device(self, tables):
        self._batch(self._lib.ecb_table_merge_batch_device, tables)

    def table_adopt_batch_device(self, tables):
        self._batch(self._lib.ecb_table_adopt_batch_device, tables)

    def table_rebase_device(self, entries, n_entries, read_base):
        """Exported entries (device tensor), in place: first reads moved on by ``read_base``; ordered ahead of a merge on this handle."""
        self._device_call((self._lib.ecb_table_rebase_device, _dev_ptr(entries), n_entries, read_base))

    def table_adopt_device(self, entries, n_entries, pairs, n_pairs):
        self._device_call((self._lib.ecb_table_adopt_device, _dev_ptr(entries), n_entries, _dev_ptr(pairs), n_pairs))

    # -- finalize per key range ----------------------------------------------
    def export_piece_device(self, indptr, indices, data, counts, firsts):
        """After finalize, on the handle that merged one key range: CSR A, the EC counts and every EC's first read (global
        index) into int32 device tensors of E + 1 / nnz / nnz / E / E elements."""
        self._device_call((self._lib.ecb_export_device, _dev_ptr(indptr), _dev_ptr(indices), _dev_ptr(data), None, None, _dev_ptr(counts)),
                          (self._lib.ecb_export_firsts_device, _dev_ptr(firsts)))

    def assemble_ranges_device(self, pieces, n_reads, all_alignments, valid_alignments):
        """``pieces``: [(indptr, indices, data, counts, firsts, n_ecs, nnz), ...] of int32 device tensors, one per key range,
        into this (empty) handle, which is finalized afterwards -> sizes."""
        k = len(pieces)
        ptrs = [(C.c_void_p * k)(*[p[i].data_ptr() for p in pieces]) for i in range(5)]
        ne, nz = (C.c_uint64 * k)(*[p[5] for p in pieces]), (C.c_uint64 * k)(*[p[6] for p in pieces])
        s = Sizes()
        self._device_call((self._lib.ecb_assemble_ranges_device, k) + tuple(ptrs) + (ne, nz, n_reads, all_alignments, valid_alignments, C.byref(s)))
        self.sizes = {k_: int(getattr(s, k_)) for k_, _ in Sizes._fields_}
        return self.sizes

    # -- multisample across GPUs ----------------------------------------------
    def export_ec_keys_device(self, keys):
        """After finalize: the 8-byte set hash of every EC in rank order into ``keys`` (int64 tensor of n_ecs)."""
        self._device_call((self._lib.ecb_export_ec_keys_device, _dev_ptr(keys)))

    def export_device(self, indptr, indices, data):
        """After finalize: CSR A into int32 device tensors of E + 1 / nnz / nnz elements."""
        self._device_call((self._lib.ecb_export_device, _dev_ptr(indptr), _dev_ptr(indices), _dev_ptr(data), None, None, None))

    def ms_local_triples_device(self, keys, indptr, indices, data, n_ecs, read_base, out_key, out_count, out_first):
        """A shard's (EC, cell, file) triples with global EC ids (its ECs found in the merged result by hash ``keys`` and
        then by key against the merged CSR rows) -> number of triples written."""
        n = C.c_uint64()
        self._device_call((self._lib.ecb_ms_local_triples_device, _dev_ptr(keys), _dev_ptr(indptr), _dev_ptr(indices), _dev_ptr(data), n_ecs,
                           read_base, _dev_ptr(out_key), _dev_ptr(out_count), _dev_ptr(out_first), C.byref(n)))
        return n.value

    def ms_adopt_triples_device(self, tables):
        """``tables``: [(key int64 tensor, count int32 tensor, first int32 tensor, n), ...] -> number of distinct triples."""
        k = len(tables)
        pk, pc = (C.c_void_p * k)(*[t[0].data_ptr() for t in tables]), (C.c_void_p * k)(*[t[1].data_ptr() for t in tables])
        pf, nn = (C.c_void_p * k)(*[t[2].data_ptr() for t in tables]), (C.c_uint64 * k)(*[t[3] for t in tables])
        out = C.c_uint64()
        self._device_call((self._lib.ecb_ms_adopt_triples_device, k, pk, pc, pf, nn, C.byref(out)))
        if self.sizes is not None:
            self.sizes["nnz_n"] = out.value
        return out.value

    def counters(self):
        """-> (all_alignments, valid_alignments, n_reads) so far."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._chk(self._lib.ecb_counters(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def add_counters(self, all_alignments, valid_alignments, n_reads):
        self._chk(self._lib.ecb_add_counters(self._h, all_alignments, valid_alignments, n_reads))

    # -- measurement ---------------------------------------------------------
    def profile(self, enable=True):
        self._chk(self._lib.ecb_profile(self._h, 1 if enable else 0))

    def profile_read(self):
        ms, n, r = C.c_double(), C.c_uint64(), C.c_uint64()
        self._chk(self._lib.ecb_profile_read(self._h, C.byref(ms), C.byref(n), C.byref(r)))
        return ms.value, n.value, r.value

    def merge_from(self, shards):
        """``ecb_merge``: this (empty) handle becomes the finalized result of the contiguous read shards held by the builders in
        ``shards`` (each on its own GPU, pushed but not finalized): the multi-GPU merge inside libecb, one process, peer copies."""
        k = len(shards)
        hs = (C.c_void_p * k)(*[b._h for b in shards])
        s = Sizes()
        self._chk(self._lib.ecb_merge(hs, k, self._h, C.byref(s)))
        self.sizes = {k_: int(getattr(s, k_)) for k_, _ in Sizes._fields_}
        return self.sizes

    def profile_kernel(self):
        """Name of the stream kernel the last batch launched (as rocprofv3 prints it)."""
        return (self._lib.ecb_profile_kernel(self._h) or b"").decode() if hasattr(self._lib, "ecb_profile_kernel") else ""
