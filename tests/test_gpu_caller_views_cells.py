"""The per-cell device entry points (``ecb_cell_support_device``, ``ecb_quantify_cells_device``; their host twins take no device memory) on
caller memory as a caller has it: offset, guarded views of one larger tensor (``tests/caller_views.py``), in the manner and with the matrices
of ``test_gpu_caller_views.py`` -- nnz(A) just above two workgroups of the four-per-thread passes at every residue modulo 4, one row longer
than a workgroup, stored masks and counts of 0, a cell of two reads.  After every call: the return code, the support bit for bit and theta
within the step's derived bound of the cell checker's -- and bit for bit the same call on aligned tensors --, and ``Slab.check()`` empty: no
guard byte touched on either side of any array (the per-cell outputs of the device entry are device arrays too), no input changed."""
import ctypes as C

import numpy as np
import pytest

from alntools_amd import ecb

import cell_quant_checker as cq
import quant_checker as qchk
from caller_views import _torch_dtype
from test_gpu_caller_views import CONTRACT, H, S, T, Case, _P, _cached, _csr_ins, _falling, _good_call, _matrix, _place

pytestmark = pytest.mark.gpu
KEEP = np.array([1, 2, 1, 1, 0, 255, 1, 1, 1, 0, 1], dtype=np.uint8)       # (non-zero = kept)


def _head(m, v):
    return (0, m.num_reads, T, H, len(m.indicesA), _P(v["ip"]), _P(v["ix"]), _P(v["da"]), S, len(m.indicesN), _P(v["pn"]), _P(v["xn"]), _P(v["dn"]),
            _P(v["keep"]))


def _cells(key):
    m = _matrix(key, 1)
    return m, _cached(("cells", key), lambda: cq.cells(m, KEEP))


def case_cell_support(key):
    m, cs = _cells(key)
    ptr, loc = cq.expected_support(cs)

    def call(v):
        ns = C.c_uint64(0xDEAD)
        rc = ecb.load().ecb_cell_support_device(*(_head(m, v) + (_P(v["cell_ptr"]), _P(v["slot_locus"]), len(loc), C.byref(ns))))
        return rc, ns.value

    def verify(out, ns):
        assert ns == len(loc) and np.array_equal(out["cell_ptr"], ptr) and np.array_equal(out["slot_locus"], loc)
    return Case(_csr_ins(m) + [("keep", KEEP, np.uint8)], [("cell_ptr", (S + 1,), np.int64), ("slot_locus", (len(loc),), np.int32)], call, verify,
                bad=("ip", _falling(m.indptrA), CONTRACT))


PER_CELL = [("n_iter", np.uint32), ("delta", np.float64), ("explained", np.int64), ("converged", np.uint8)]


def case_quantify_cells(key):
    """One step (``max_iters=1``, ``tol=0``) of every kept cell from one shared theta with a scale."""
    import torch
    m, cs = _cells(key)
    ptr, loc = cq.expected_support(cs)
    rng = np.random.default_rng(40 + key)
    theta_in = rng.random((H, T)) * 10 + 0.01
    theta_in[:, m.indicesA[m.indptrA[5]:m.indptrA[6]]] = 0.0             # (a row whose targets all have theta = 0)
    scale = 1.0 / rng.integers(1, 3000, size=(H, T))
    refs = [None if c is None else c.step(theta_in, scale) for c in cs]
    outs = [("cell_ptr", (S + 1,), np.int64), ("slot_locus", (len(loc),), np.int32), ("theta", (len(loc), H), np.float64)] + [(n, (S,), dt) for n, dt in PER_CELL]

    def call(v):
        rc = ecb.load().ecb_quantify_cells_device(*(_head(m, v) + (_P(v["scale"]), _P(v["theta_in"]), 1, 0.0, 0, len(loc)) + tuple(_P(v[o[0]]) for o in outs)))
        return rc, None

    def aligned():
        v = {n: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda() for n, a, dt in _csr_ins(m) + [("keep", KEEP, np.uint8)]}
        v.update(scale=torch.from_numpy(scale).cuda(), theta_in=torch.from_numpy(theta_in).cuda())
        for n, shape, dt in outs:
            v[n] = torch.zeros(shape, dtype=_torch_dtype(np.dtype(dt)), device="cuda")
        assert all(t.data_ptr() % 16 == 0 for t in v.values())
        assert call(v)[0] == 0
        torch.cuda.synchronize()
        return {n: v[n].cpu().numpy().tobytes() for n, _, _ in outs}
    plain = _cached(("cells_aligned", key), aligned)

    def verify(out, _):
        assert np.array_equal(out["cell_ptr"], ptr) and np.array_equal(out["slot_locus"], loc)
        for c, cell in enumerate(cs):
            if cell is None or cell.empty():
                assert ptr[c] == ptr[c + 1] and (out["n_iter"][c], out["delta"][c], out["explained"][c], out["converged"][c]) == (0, 0.0, 0, 1)
                continue
            qchk.agree(cell.scatter(out["theta"][ptr[c]:ptr[c + 1]]), refs[c][0], cell.tolerance())
            assert out["n_iter"][c] == 1 and out["explained"][c] == refs[c][1]
        assert all(out[n].tobytes() == plain[n] for n, _, _ in outs)
    bad = scale.copy()
    bad[1, T // 2] = np.nan
    return Case(_csr_ins(m) + [("keep", KEEP, np.uint8), ("scale", scale, np.float64), ("theta_in", theta_in, np.float64)], outs, call, verify,
                bad=("scale", bad, CONTRACT))


CSR_N = ["ip", "ix", "da", "pn", "xn", "dn"]
ENTRIES = {
    "cell_support": (case_cell_support, CSR_N + ["keep", "cell_ptr", "slot_locus"]),
    "quantify_cells": (case_quantify_cells, CSR_N + ["keep", "scale", "theta_in", "cell_ptr", "slot_locus", "theta"] + [n for n, _ in PER_CELL]),
}
#: every residue of nnz(A) modulo 4 under the four placements of all arrays; each array alone off 16 bytes at one of them
PLACED = [(e, k, p) for e in ENTRIES for k in (0, 1, 2, 3) for p in ("control", "all4", "all8", "all12")] + \
         [(e, 1, "one:" + n) for e, (_, names) in ENTRIES.items() for n in names]


def _case(entry, key):
    return _cached(("cells_case", entry, key), lambda: ENTRIES[entry][0](key))


@pytest.mark.parametrize("entry,key,placement", PLACED, ids=["%s-%s-%s" % c for c in PLACED])
def test_the_cell_entry_points_on_offset_guarded_views(entry, key, placement):
    case = _case(entry, key)
    assert case.names == ENTRIES[entry][1]
    slab, v = _place(case, placement)
    if placement != "control":
        assert any(t.data_ptr() % 16 for t in v.values())
    _good_call(case, slab, v)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_a_refused_call_on_offset_views_leaves_the_outputs_and_the_guards_alone(entry):
    import torch
    case = _case(entry, 1)
    name, bad, code = case.bad
    slab, v = _place(case, "all4", extra=[(name + "~bad", bad, next(dt for n, _, dt in case.ins if n == name))])
    rc, _ = case.call(dict(v, **{name: v[name + "~bad"]}))
    torch.cuda.synchronize()
    assert rc == code, (rc, ecb.load().ecb_last_error(None))
    host = slab.host()
    for out, _, _ in case.outs:
        assert slab.untouched(out, host), out
    assert slab.check(host) == []
    _good_call(case, slab, v)
