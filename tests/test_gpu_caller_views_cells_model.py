"""The per-cell model device entry point (``ecb_quantify_cells_model_device``; its host twin takes no device memory) on caller memory as a
caller has it: offset, guarded views of one larger tensor (``tests/caller_views.py``), in the manner and with the matrices of
``test_gpu_caller_views_cells.py``, ``gene`` among the placed arrays, for every model.  After every call: the return code, the support bit
for bit and theta within the step's derived bound of the cell model checker's -- and bit for bit the same call on aligned tensors --, and
``Slab.check()`` empty: no guard byte touched on either side of any array, no input changed."""
import numpy as np
import pytest

from alntools_amd import ecb

import cell_model_checker as cm
import cell_quant_checker as cq
import quant_checker as qchk
from caller_views import _torch_dtype
from test_gpu_caller_views import CONTRACT, H, S, T, Case, _P, _cached, _csr_ins, _good_call, _matrix, _place
from test_gpu_caller_views_cells import KEEP, PER_CELL, _head

pytestmark = pytest.mark.gpu
N_GENES = 40


def _cells(key):
    m = _matrix(key, 1)
    gene = np.random.default_rng(7 + key).integers(0, N_GENES, size=T).astype(np.int32)          # (ids interleave in locus order)
    return m, gene, _cached(("cells_model", key), lambda: cm.groupings(cq.cells(m, KEEP), gene, N_GENES))


def case_quantify_cells_model(key, model):
    """One step (``max_iters=1``, ``tol=0``) of every kept cell from one shared theta with a scale."""
    import torch
    m, gene, qs = _cells(key)
    ptr, loc = cq.expected_support([None if q is None else q.cell for q in qs])
    rng = np.random.default_rng(40 + key)
    theta_in = rng.random((H, T)) * 10 + 0.01
    theta_in[:, m.indicesA[m.indptrA[5]:m.indptrA[6]]] = 0.0             # (a row whose targets all have theta = 0)
    scale = 1.0 / rng.integers(1, 3000, size=(H, T))
    refs = [None if q is None else q.step(model, theta_in, scale) for q in qs]
    ins = _csr_ins(m) + [("keep", KEEP, np.uint8), ("scale", scale, np.float64), ("theta_in", theta_in, np.float64), ("gene", gene, np.int32)]
    outs = [("cell_ptr", (S + 1,), np.int64), ("slot_locus", (len(loc),), np.int32), ("theta", (len(loc), H), np.float64)] + [(n, (S,), dt) for n, dt in PER_CELL]

    def call(v):
        rc = ecb.load().ecb_quantify_cells_model_device(*(_head(m, v) + (_P(v["scale"]), _P(v["theta_in"]), 1, 0.0, 0, N_GENES, _P(v["gene"]), model, len(loc))
                                                          + tuple(_P(v[o[0]]) for o in outs)))
        return rc, None

    def aligned():
        v = {n: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda() for n, a, dt in ins}
        for n, shape, dt in outs:
            v[n] = torch.zeros(shape, dtype=_torch_dtype(np.dtype(dt)), device="cuda")
        assert all(t.data_ptr() % 16 == 0 for t in v.values())
        assert call(v)[0] == 0
        torch.cuda.synchronize()
        return {n: v[n].cpu().numpy().tobytes() for n, _, _ in outs}
    plain = _cached(("cells_model_aligned", key, model), aligned)

    def verify(out, _):
        assert np.array_equal(out["cell_ptr"], ptr) and np.array_equal(out["slot_locus"], loc)
        for c, q in enumerate(qs):
            if q is None or q.cell.empty():
                assert ptr[c] == ptr[c + 1] and (out["n_iter"][c], out["delta"][c], out["explained"][c], out["converged"][c]) == (0, 0.0, 0, 1)
                continue
            qchk.agree(q.cell.scatter(out["theta"][ptr[c]:ptr[c + 1]]), refs[c][0], q.tolerance(model))
            assert out["n_iter"][c] == 1 and out["explained"][c] == refs[c][1]
        assert all(out[n].tobytes() == plain[n] for n, _, _ in outs)
    bad = gene.copy()
    bad[T // 2] = N_GENES
    return Case(ins, outs, call, verify, bad=("gene", bad, CONTRACT))


NAMES = ["ip", "ix", "da", "pn", "xn", "dn", "keep", "scale", "theta_in", "gene", "cell_ptr", "slot_locus", "theta"] + [n for n, _ in PER_CELL]
MODELS = (1, 2, 3)
#: every residue of nnz(A) modulo 4 under the four placements of all arrays, for every model; each array alone off 16 bytes at one of them
PLACED = [(model, k, p) for model in MODELS for k in (0, 1, 2, 3) for p in ("control", "all4", "all8", "all12")] + \
         [(model, 1, "one:" + n) for model in MODELS for n in NAMES]


def _case(model, key):
    return _cached(("cells_model_case", model, key), lambda: case_quantify_cells_model(key, model))


@pytest.mark.parametrize("model,key,placement", PLACED, ids=["m%d-%s-%s" % c for c in PLACED])
def test_the_cell_model_entry_point_on_offset_guarded_views(model, key, placement):
    case = _case(model, key)
    assert case.names == NAMES
    slab, v = _place(case, placement)
    if placement != "control":
        assert any(t.data_ptr() % 16 for t in v.values())
    _good_call(case, slab, v)


@pytest.mark.parametrize("model", MODELS + (4,))
def test_a_gene_id_out_of_range_on_offset_views_leaves_the_outputs_and_the_guards_alone(model):
    import torch
    case = _case(model if model != 4 else 1, 1)
    name, bad, code = case.bad
    slab, v = _place(case, "all4", extra=[(name + "~bad", bad, np.int32)])
    lib = ecb.load()
    m = _cells(1)[0]
    outs = tuple(_P(v[o[0]]) for o in case.outs)
    rc = lib.ecb_quantify_cells_model_device(*(_head(m, v) + (_P(v["scale"]), _P(v["theta_in"]), 1, 0.0, 0, N_GENES, _P(v[name + "~bad"]), model,
                                                              case.outs[1][1][0]) + outs))
    torch.cuda.synchronize()
    assert rc == code, (rc, lib.ecb_last_error(None))
    host = slab.host()
    for out, _, _ in case.outs:
        assert slab.untouched(out, host), out
    assert slab.check(host) == []
    _good_call(case, slab, v)
