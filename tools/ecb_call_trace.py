#!/usr/bin/env python
"""What every one-call wrapper of ``alntools_amd/ecb.py`` hands to libecb, recorded on the CPU with a stand-in for the library.

    python tools/ecb_call_trace.py trace [--tree DIR] [--out FILE]    the trace: its sha256 and the number of library calls
    python tools/ecb_call_trace.py time  [--tree DIR]                 the wrappers' own time per call against a no-op library
    python tools/ecb_call_trace.py digest [--tree DIR] [--out FILE]   on a GPU, with the built library: a sha256 per returned array

``--tree``: the checkout whose ``alntools_amd`` is driven (default: this one), so that two commits can be compared by the same driver.
The stand-in is installed as ``ecb._lib``; no GPU and no built library are needed.  ``np.empty`` / ``torch.empty`` are made to fill
their result with 0xA5 while the trace runs, so that the bytes of every buffer -- zeroed or not -- are the same from run to run.
Tensors are CPU tensors (they have ``data_ptr()``; their device index counts as 0)."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "..", "tests", "golden")
CASES = (("g2_c1.bin", "quant_model_c1.grp.txt", "bundle_c1_mixed.grp.txt"), ("g4b_multi_min0.bin", "quant_model_ms.grp.txt", "gt_ms.grp.txt"))
WRITES = {"ecb_csr_to_hapcsc": (3,), "ecb_csr_to_hapcsc_values": (3,), "ecb_hapcsc_to_csr": (2,), "ecb_apply_mask": (2,),
          "ecb_cell_support": (4,), "ecb_quantify": (7, 0.5, 11, 1), "ecb_quantify_model": (7, 0.5, 11, 1),
          "ecb_combine": (1, 2, 2), "ecb_bundle": (1, 2, 2), "ecb_select": (1, 2, 1, 2), "ecb_salmon_ecs": (2, 1)}


def sha(b):
    return hashlib.sha256(b).hexdigest()[:16]


def as_bytes(a):
    return (a.contiguous().cpu().numpy() if hasattr(a, "data_ptr") else np.ascontiguousarray(a)).tobytes()


def describe_array(a):
    kind = "torch" if hasattr(a, "data_ptr") else "numpy"
    return [kind, str(a.dtype), list(a.shape), sha(as_bytes(a))]


def address(a):
    return a.data_ptr() if hasattr(a, "data_ptr") else a.__array_interface__["data"][0]


def live_arrays():
    """Every array a frame between the library call and this driver holds in a local, a list, a tuple or a dict."""
    found, f = [], sys._getframe(2)

    def collect(v, depth):
        if isinstance(v, np.ndarray) or hasattr(v, "data_ptr"):
            found.append(v)
        elif depth and isinstance(v, (list, tuple)):
            for x in v:
                collect(x, depth - 1)
        elif depth and isinstance(v, dict):
            for x in v.values():
                collect(x, depth - 1)
    here = os.path.abspath(__file__)
    while os.path.abspath(f.f_code.co_filename) == here:       # (the stand-in's own frames)
        f = f.f_back
    while f is not None and os.path.abspath(f.f_code.co_filename) != here:
        for v in list(f.f_locals.values()):
            collect(v, 2)
        f = f.f_back
    return found


def resolve(addr, arrays):
    """The largest live array that starts at ``addr``."""
    hits = [a for a in arrays if address(a) == addr]
    if not hits:
        return None
    return max(hits, key=lambda a: a.numel() * a.element_size() if hasattr(a, "data_ptr") else a.nbytes)


class StandIn(object):
    """``ecb._lib``: one recording method per symbol of the headers; every call returns ``fail[0]`` (0 unless a case sets it)."""

    def __init__(self, ecb, record=True):
        self.calls, self.record, self.tot, self.fail = [], record, None, (0, b"")
        names = sum((getattr(ecb, n) for n in dir(ecb) if n == "SYMBOLS" or n.endswith("_SYMBOLS")), ())
        for n in names:
            if n != "ecb_last_error":
                setattr(self, n, (lambda *a, _n=n: self._call(_n, a)))

    def ecb_last_error(self, h):
        return self.fail[1]

    def _describe(self, a, arrays):
        if a is None or isinstance(a, (bool, int, float)):
            return a
        if isinstance(a, C.c_void_p):
            if not a.value:
                return "null"
            hit = resolve(a.value, arrays)
            assert hit is not None, "a pointer to no live array"
            return describe_array(hit)
        if hasattr(a, "_obj"):
            return ["byref", type(a._obj).__name__]
        if isinstance(a, C.Array):
            if issubclass(a._type_, C.Structure):
                return [[[n, self._describe(C.c_void_p(getattr(s, n)) if t is C.c_void_p else getattr(s, n), arrays)]
                         for n, t in s._fields_] for s in a]
            return ["carray", a._type_.__name__, len(a)]
        raise TypeError("argument of type %s" % type(a).__name__)

    def _call(self, name, args):
        base = name[:-7] if name.endswith("_device") else name
        arrays = live_arrays() if self.record or base == "ecb_cell_support" else []
        if self.record:
            self.calls.append([name] + [self._describe(a, arrays) for a in args])
        if self.fail[0]:
            return self.fail[0]
        vals = WRITES.get(base, ())
        if base.startswith("ecb_csr_to_hapcsc") and self.tot is not None:
            vals = (self.tot,)
        if isinstance(args[-1], C.Array):
            for i, v in enumerate(vals):
                args[-1][i] = v
        else:
            for a, v in zip(args[len(args) - len(vals):], vals):
                a._obj.value = v
        if base == "ecb_cell_support" and arrays:                # (cell_ptr: quantify_cells sizes its buffers by the last entry)
            cell_ptr = resolve(args[14].value, arrays)
            cell_ptr[:] = 0
            cell_ptr[-1] = 4
        return 0


def poisoned(empty, view):
    def f(*a, **k):
        out = empty(*a, **k)
        view(out).fill(0xA5) if empty is np_empty else view(out).fill_(0xA5)
        return out
    return f


np_empty, torch_empty = np.empty, torch.empty


def describe_result(r):
    if isinstance(r, (tuple, list)):
        return [describe_result(x) for x in r]
    if isinstance(r, dict):
        return [[k, describe_result(v)] for k, v in sorted(r.items())]
    if isinstance(r, np.ndarray) or hasattr(r, "data_ptr"):
        return describe_array(r)
    return [type(r).__name__, r if r is None or isinstance(r, (bool, int, float, str)) else repr(r)]


def inputs(tree_bin_utils, tensors, wide, ecb=None):
    """Per golden file: the matrices, sizes and side arrays of one kind (``wide``: int64 where the wrappers convert to int32).  ``ecb``: for
    the built library (tensors on the GPU; what the stand-in lets be anything is made what the library expects)."""
    where = "cuda" if ecb is not None else "cpu"
    conv = (lambda a, dt=None: torch.as_tensor(np.array(a, dtype=dt)).to(where)) if tensors else (lambda a, dt=None: np.array(a, dtype=dt))
    idt = np.int64 if wide else np.int32
    for ec, grp, bgrp in CASES:
        m = tree_bin_utils.ecload(os.path.join(GOLDEN, ec))
        gene, names = tree_bin_utils.gene_ids(m, os.path.join(GOLDEN, grp))
        gname, map_ptr, map_idx, _ = tree_bin_utils.group_map(m, os.path.join(GOLDEN, bgrp))
        T, H, S, E = m.num_loci, m.num_haplotypes, m.num_samples, m.num_reads
        rng = np.random.RandomState(7)
        d = dict(A=[conv(x, idt) for x in (m.indptrA, m.indicesA, m.dataA)], N=[conv(x, idt) for x in (m.indptrN, m.indicesN, m.dataN)],
                 T=T, H=H, S=S, E=E, gene=conv(gene, idt), gene_np=gene, n_genes=len(names), n_groups=len(gname),
                 map_ptr=conv(map_ptr, idt), map_idx=conv(map_idx, idt), scale=conv(rng.rand(H, T), np.float64),
                 theta=conv(rng.rand(H, T) + 1, np.float64), keep=conv(np.arange(S) % 2 == 0), values=conv(rng.rand(5), np.float64),
                 mask=conv(rng.randint(0, 1 << H, T), np.int32 if tensors else (np.int64 if wide else np.uint32)),
                 cptr=conv(np.minimum(np.arange(H * (T + 1)), 6).reshape(H, T + 1), idt), cidx=conv(np.arange(6) % E, idt),
                 tmap=conv(np.arange(T)[::-1].copy(), np.int64), smap=conv(np.arange(S), np.int64), conv=conv, n_slots={False: 6, True: 6})
        if ecb is not None:
            mats = (m.indptrA, m.indicesA, m.dataA, T, H, m.indptrN, m.indicesN, m.dataN)
            cptr, cidx = ecb.csr_to_hapcsc_host(m.indptrA, m.indicesA, m.dataA, T, H)
            d.update(values=conv(rng.rand(len(cidx)), np.float64), cptr=conv(cptr, idt), cidx=conv(cidx, idt),
                     n_slots={k: int(ecb.cell_support(*mats, cell_keep=keep, count_only=True)[0][-1])
                              for k, keep in ((False, None), (True, np.arange(S) % 2 == 0))})
        yield ec, d


def calls_of(ecb, d, tensors, lib, real=False):
    """(label, thunk) for every wrapper, each optional argument absent and present (``real``: the cases for the built library on one GPU)."""
    dv = 0 if real else 1
    A, N, T, H, S, E, conv = d["A"], d["N"], d["T"], d["H"], d["S"], d["E"], d["conv"]
    mats = (A[0], A[1], A[2], T, H, N[0], N[1], N[2])
    six = (A[0], A[1], A[2], N[0], N[1], N[2])
    short = A[2][:-1]
    bad_tab, bad_gene, bad_keep = d["scale"][:, :-1], d["gene"][:-1], d["keep"][:-1]
    out = []

    def add(label, fn, *a, **k):
        out.append((label, lambda: fn(*a, **k)))

    def tot(n, fn, *a, **k):
        def run():
            lib.tot = n
            try:
                return fn(*a, **k)
            finally:
                lib.tot = None
        return run
    if tensors:                                       # (the conversions take int32 tensors as they are)
        A32, cptr32, cidx32 = [a.to(torch.int32) for a in A], d["cptr"].to(torch.int32), d["cidx"].to(torch.int32)
        add("csr_to_hapcsc", ecb.csr_to_hapcsc, *A32, T, H)
        add("csr_to_hapcsc nnz", ecb.csr_to_hapcsc, *A32, T, H, nnz=len(A32[1]) if real else 11)
        add("csr_to_hapcsc count first", ecb.csr_to_hapcsc, *A32, T, H, nnz=1 << 28)
        out.append(("csr_to_hapcsc_values", tot(5, ecb.csr_to_hapcsc_values, *A32, d["values"], T, H)))
        out.append(("csr_to_hapcsc_values mismatch", tot(4, ecb.csr_to_hapcsc_values, *A32, d["values"], T, H)))
        add("hapcsc_to_csr", ecb.hapcsc_to_csr, cptr32, cidx32, E)
        add("hapcsc_to_csr empty", ecb.hapcsc_to_csr, cptr32, cidx32[:0], E)
    else:
        for dev in (0, dv):
            add("csr_to_hapcsc_host %d" % dev, ecb.csr_to_hapcsc_host, *A, T, H, dev)
            out.append(("csr_to_hapcsc_values_host %d" % dev, tot(5, ecb.csr_to_hapcsc_values_host, *A, d["values"], T, H, dev)))
            add("hapcsc_to_csr_host %d" % dev, ecb.hapcsc_to_csr_host, d["cptr"], d["cidx"], E, dev)
        out.append(("csr_to_hapcsc_values_host mismatch", tot(4, ecb.csr_to_hapcsc_values_host, *A, d["values"], T, H)))
        add("hapcsc_to_csr_host empty", ecb.hapcsc_to_csr_host, d["cptr"], d["cidx"][:0], E)
    add("apply_mask", ecb.apply_mask, *A, d["mask"], H)
    add("apply_mask device", ecb.apply_mask, *A, d["mask"], H, device=dv)
    add("apply_mask short", ecb.apply_mask, A[0], A[1], short, d["mask"], H)
    for sample in (None, 0, S - 1):
        add("count_alignments %s" % sample, ecb.count_alignments, *mats, sample=sample, device=dv)
        for scale in (None, d["scale"]):
            for theta in (None, d["theta"]):
                lab = "%s %s %s" % (sample, scale is not None, theta is not None)
                add("quantify " + lab, ecb.quantify, *mats, sample=sample, scale=scale, theta_in=theta, max_iters=9, tol=1e-3)
                add("quantify_model " + lab, ecb.quantify_model, *mats, d["gene"], d["n_genes"], 1 + (sample or 0) % 4, sample=sample, scale=scale,
                    theta_in=theta, device=dv)
    add("count_alignments short", ecb.count_alignments, A[0], A[1], short, T, H, *N)
    add("quantify defaults", ecb.quantify, *mats)
    add("quantify_model numpy gene", ecb.quantify_model, *mats, d["gene_np"], d["n_genes"], 2)
    add("quantify short", ecb.quantify, A[0], A[1], A[2], T, H, N[0], N[1], N[2][:-1], scale=bad_tab)
    add("quantify_model gene then tables", ecb.quantify_model, *mats, bad_gene, d["n_genes"], 2, scale=bad_tab)
    add("quantify_model tables", ecb.quantify_model, *mats, d["gene"], d["n_genes"], 2, theta_in=bad_tab)
    for scale in (None, d["scale"]):
        for gene, n_genes, model in ((None, 0, 4), (d["gene"], d["n_genes"], 4), (d["gene"], d["n_genes"], 1), (d["gene_np"], d["n_genes"], 3)):
            add("posterior %s %s %d" % (scale is not None, gene is not None, model), ecb.posterior, A[0], A[1], A[2], T, H, d["theta"], scale=scale,
                gene=gene, n_genes=n_genes, model=model, device=dv)
    add("posterior defaults", ecb.posterior, A[0], A[1], A[2], T, H, d["theta"])
    add("posterior no bits", ecb.posterior, A[0], A[1], A[2] * 0, T, H, d["theta"])
    add("posterior no theta", ecb.posterior, A[0], A[1], A[2], T, H, None, scale=d["scale"])
    add("posterior short", ecb.posterior, A[0], A[1], short, T, H, bad_tab, gene=bad_gene)
    add("posterior tables then gene", ecb.posterior, A[0], A[1], A[2], T, H, bad_tab, gene=bad_gene)
    add("posterior gene", ecb.posterior, A[0], A[1], A[2], T, H, d["theta"], gene=bad_gene)
    for keep in (None, d["keep"]):
        for count_only in (False, True):
            add("cell_support %s %s" % (keep is not None, count_only), ecb.cell_support, *mats, cell_keep=keep, device=dv, count_only=count_only)
        for scale in (None, d["scale"]):
            for theta in (None, d["theta"]):
                for n_slots in (None, d["n_slots"][keep is not None]):
                    lab = "%s %s %s %s" % (keep is not None, scale is not None, theta is not None, n_slots)
                    add("quantify_cells " + lab, ecb.quantify_cells, *mats, cell_keep=keep, scale=scale, theta_in=theta, max_iters=5, tol=1e-2,
                        budget_bytes=150000 if n_slots else 0, device=dv, n_slots=n_slots)
                    add("quantify_cells_model " + lab, ecb.quantify_cells_model, *mats, d["gene"], d["n_genes"], 3, cell_keep=keep, scale=scale,
                        theta_in=theta, n_slots=n_slots)
    add("cell_support list keep", ecb.cell_support, *mats, cell_keep=[1] * S)
    add("cell_support short", ecb.cell_support, A[0], A[1], short, T, H, *N, cell_keep=bad_keep)
    add("cell_support keep", ecb.cell_support, *mats, cell_keep=bad_keep)
    add("quantify_cells defaults", ecb.quantify_cells, *mats)
    add("quantify_cells keep then tables", ecb.quantify_cells, *mats, cell_keep=bad_keep, scale=bad_tab)
    add("quantify_cells_model tables then gene", ecb.quantify_cells_model, *mats, bad_gene, d["n_genes"], 1, scale=bad_tab)
    add("quantify_cells_model gene", ecb.quantify_cells_model, *mats, bad_gene, d["n_genes"], 1)
    keys = ("indptrA", "indicesA", "dataA", "indptrN", "indicesN", "dataN")
    part = dict(zip(keys, six), n_loci=T, target_map=None, sample_map=d["smap"])
    mapped = dict(part, target_map=d["tmap"])
    plain = dict(zip(keys, six), n_loci=T)
    add("combine", ecb.combine, [part, mapped] + ([] if real else [plain]), T, H, S, device=dv)
    add("combine one", ecb.combine, [mapped], T, H, S)
    add("combine none", ecb.combine, [], T, H, S)
    add("combine short", ecb.combine, [part, dict(part, dataN=N[2][:-1])], T, H, S)
    add("bundle", ecb.bundle, *six, T, H, d["n_groups"], d["map_ptr"], d["map_idx"], device=dv)
    add("bundle defaults", ecb.bundle, *six, T, H, d["n_groups"], d["map_ptr"], d["map_idx"])
    add("bundle short", ecb.bundle, A[0], A[1], short, *N, T, H, d["n_groups"], d["map_ptr"], d["map_idx"])
    add("bundle map", ecb.bundle, *six, T, H, d["n_groups"], d["map_ptr"][:-1], d["map_idx"])
    for row_class in (None, "all", "unique", "locus-unique", "multi", 2):
        for keep in (None, d["keep"]):
            for min_count in (None, 3, -2):
                add("select %s %s %s" % (row_class, keep is not None, min_count), ecb.select, *six, T, H, row_class=row_class, sample_keep=keep,
                    min_count=min_count, device=dv)
    add("select defaults", ecb.select, *six, T, H)
    add("select list keep", ecb.select, *six, T, H, sample_keep=[0, 1] * (S // 2) + [1] * (S % 2))
    add("select short", ecb.select, A[0], A[1], short, *N, T, H, sample_keep=bad_keep)
    add("select keep", ecb.select, *six, T, H, sample_keep=bad_keep)
    text = b"2\t0\t1\t5\n1\t2\t0\n3\t0\t1\t2\t7\n"
    col, hap = np.array([0, 1, 1]), np.array([0, 0, 1])
    texts = [("tensor", torch.as_tensor(np.frombuffer(text, dtype=np.uint8).copy()).to(A[0].device))] if tensors else \
        [("bytes", text), ("array", np.frombuffer(text, dtype=np.uint8)), ("bytearray", bytearray(text))]
    for lab, t in texts:
        add("salmon_ecs " + lab, ecb.salmon_ecs, t, 3, col, hap, 2, 2, device=dv)
        add("salmon_ecs %s lists" % lab, ecb.salmon_ecs, t, 3, [0, 1, 1], [0, 0, 1], 2, 2)
        add("salmon_ecs %s few tabs" % lab, ecb.salmon_ecs, t, 40, col.astype(np.uint32), hap.astype(np.int32), 2, 2)

        def refused(rc, msg, t=t):
            lib.fail = (rc, msg)
            try:
                return ecb.salmon_ecs(t, 3, col, hap, 2, 2)
            finally:
                lib.fail = (0, b"")
        if real:
            continue
        out.append(("salmon_ecs %s format" % lab, lambda r=refused: r(-5, b"EC line 1: k differs (reason 5)")))
        out.append(("salmon_ecs %s contract" % lab, lambda r=refused: r(-5, b"something else")))
        out.append(("salmon_ecs %s limit" % lab, lambda r=refused: r(-8, b"EC line 1: too large (reason 3)")))
    if not tensors:
        add("salmon_ecs lengths", ecb.salmon_ecs, text, 3, col, hap[:-1], 2, 2)

    def failing():
        lib.fail = (-5, b"refused")
        try:
            return ecb.apply_mask(*A, d["mask"], H)
        finally:
            lib.fail = (0, b"")
    if real:            # (no case whose answer rests on how the library treats what it is not meant to be handed)
        return [(lab, th) for lab, th in out if not lab.endswith((" empty", " no bits", "combine none", " few tabs"))]
    out.append(("apply_mask refused", failing))
    return out


def load_tree(tree):
    sys.path.insert(0, os.path.abspath(tree))
    from alntools_amd import bin_utils, ecb
    assert os.path.abspath(ecb.__file__).startswith(os.path.abspath(tree)), ecb.__file__
    return ecb, bin_utils


def trace(ecb, bin_utils, out):
    lib = ecb._lib = StandIn(ecb)
    np.empty = poisoned(np_empty, lambda a: a.reshape(-1).view(np.uint8))
    torch.empty = poisoned(torch_empty, lambda t: t.view(-1).view(torch.uint8))
    lines = []
    try:
        for tensors in (False, True):
            for wide in (False, True):
                for ec, d in inputs(bin_utils, tensors, wide):
                    for label, thunk in calls_of(ecb, d, tensors, lib):
                        first = len(lib.calls)
                        try:
                            result = ["returned", describe_result(thunk())]
                        except (ValueError, ecb.EcbError) as e:
                            result = ["raised", type(e).__name__, str(e)] + [getattr(e, n) for n in ("code", "line", "reason") if hasattr(e, n)]
                        lines.append(json.dumps([ec, "torch" if tensors else "numpy", "int64" if wide else "int32", label, lib.calls[first:], result]))
    finally:
        np.empty, torch.empty = np_empty, torch_empty
    text = "\n".join(lines) + "\n"
    if out:
        with open(out, "w") as fh:
            fh.write(text)
    print("wrapper calls: %d   library calls: %d   sha256 of the trace: %s" % (len(lines), len(lib.calls), hashlib.sha256(text.encode()).hexdigest()))


def digest(ecb, bin_utils, out):
    """Every case through the built library: what each call returned (or raised), one sha256 per array."""
    import types
    lib, lines = types.SimpleNamespace(tot=None, fail=(0, b"")), []
    for tensors in (False, True):
        for wide in (False, True):
            for ec, d in inputs(bin_utils, tensors, wide, ecb):
                for label, thunk in calls_of(ecb, d, tensors, lib, real=True):
                    try:
                        result = ["returned", describe_result(thunk())]
                    except (ValueError, ecb.EcbError) as e:
                        result = ["raised", type(e).__name__, str(e)]
                    lines.append(json.dumps([ec, "torch" if tensors else "numpy", "int64" if wide else "int32", label, result]))
    text = "\n".join(lines) + "\n"
    if out:
        with open(out, "w") as fh:
            fh.write(text)
    print("wrapper calls: %d (%d refused)   sha256 of the digests: %s" % (len(lines), sum('"raised"' in ln for ln in lines),
                                                                        hashlib.sha256(text.encode()).hexdigest()))


def timing(ecb, bin_utils, batches=9, per_batch=40):
    """Per wrapper and kind: the mean time of a call in each of ``batches`` batches -> their minimum and spread (max - min), microseconds."""
    lib = ecb._lib = StandIn(ecb, record=False)
    for tensors in (False, True):
        ec, d = next(inputs(bin_utils, tensors, False))
        seen = set()
        for label, thunk in calls_of(ecb, d, tensors, lib):
            name = label.split()[0]
            if name in seen or label.split()[-1] in ("short", "mismatch"):
                continue
            seen.add(name)
            means = []
            for _ in range(batches):
                t0 = time.perf_counter()
                for _ in range(per_batch):
                    thunk()
                means.append((time.perf_counter() - t0) / per_batch * 1e6)
            print("%-6s %-28s min %8.1f us   spread %7.1f us" % ("torch" if tensors else "numpy", name, min(means), max(means) - min(means)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("trace", "time", "digest"))
    ap.add_argument("--tree", default=os.path.join(HERE, ".."))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ecb_, bin_utils_ = load_tree(a.tree)
    {"trace": lambda: trace(ecb_, bin_utils_, a.out), "digest": lambda: digest(ecb_, bin_utils_, a.out), "time": lambda: timing(ecb_, bin_utils_)}[a.mode]()
