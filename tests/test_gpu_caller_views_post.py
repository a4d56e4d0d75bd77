"""The posterior's and the value-carrying transposition's device entry points (``ecb_posterior_device``,
``ecb_csr_to_hapcsc_values_device``; their host twins take no device memory) on caller memory as a caller has it: offset, guarded views of
one larger tensor (``tests/caller_views.py``), in the manner and with the matrices of ``test_gpu_caller_views.py`` -- every residue modulo
16 the element types allow (4-byte arrays at 0, 4, 8, 12; 8-byte arrays at 0 and 8), all arrays at once and each alone.  After every call:
the return code, the result against the checker (the posterior within its derived bound, and bit for bit the same call on aligned
tensors; the transposition exactly), and ``Slab.check()`` empty: no guard byte touched on either side of any array, no input changed."""
import ctypes as C

import numpy as np
import pytest

from alntools_amd import ecb

import post_checker as pchk
import quant_checker as qchk
import quant_model_checker as mchk
from caller_views import _torch_dtype
from test_gpu_caller_views import CONTRACT, H, T, Case, _P, _cached, _conv_matrix, _csr_ins, _falling, _good_call, _matrix, _place

pytestmark = pytest.mark.gpu
N_GENES = 40


def _call_posterior(m, v, model, n_bits, gene="gene"):
    rc = ecb.load().ecb_posterior_device(0, m.num_reads, T, H, len(m.indicesA), _P(v["ip"]), _P(v["ix"]), _P(v["da"]), _P(v["scale"]), _P(v["theta"]),
                                         N_GENES, _P(v[gene]), model, n_bits, _P(v["post"]), _P(v["bit_ptr"]), _P(v["mass"]))
    return rc, None


def case_posterior(key, model):
    """The posterior at one theta with a scale, stored masks of 0 in the matrix, one row whose targets all have theta = 0."""
    import torch
    m = _matrix(key, 1)
    gene = np.random.default_rng(7 + key).integers(0, N_GENES, size=T).astype(np.int32)
    rng = np.random.default_rng(60 + key)
    theta = rng.random((H, T)) * 10 + 0.01
    theta[:, m.indicesA[m.indptrA[5]:m.indptrA[6]]] = 0.0
    scale = 1.0 / rng.integers(1, 3000, size=(H, T))
    q = mchk.Grouping(qchk.Problem.of(m), gene, N_GENES)
    lay = pchk.Layout.of(m)
    ref, ref_mass = pchk.posterior(q, lay, model, theta, scale)
    bound, mass_bound = pchk.tolerance(model, q.p.B, H, q.M, q.R), pchk.tolerance(4, q.p.B, H)
    ins = _csr_ins(m, n=False) + [("scale", scale, np.float64), ("theta", theta, np.float64), ("gene", gene, np.int32)]
    outs = [("post", (lay.n_bits,), np.float64), ("bit_ptr", (lay.nnz + 1,), np.int64), ("mass", (lay.E,), np.float64)]

    def aligned():
        v = {n: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda() for n, a, dt in ins}
        for n, shape, dt in outs:
            v[n] = torch.zeros(shape, dtype=_torch_dtype(np.dtype(dt)), device="cuda")
        assert all(t.data_ptr() % 16 == 0 for t in v.values())
        assert _call_posterior(m, v, model, lay.n_bits)[0] == 0
        torch.cuda.synchronize()
        return {n: v[n].cpu().numpy().tobytes() for n, _, _ in outs}
    plain = _cached(("post_aligned", key, model), aligned)

    def verify(out, _):
        qchk.agree(out["post"], ref, bound)
        qchk.agree(out["mass"], ref_mass, mass_bound)
        assert np.array_equal(out["bit_ptr"], lay.bit_ptr) and out["mass"][5] == 0.0
        assert all(out[n].tobytes() == plain[n] for n, _, _ in outs)
    bad = theta.copy()
    bad[1, T // 2] = np.nan
    return Case(ins, outs, lambda v: _call_posterior(m, v, model, lay.n_bits), verify, bad=("theta", bad, CONTRACT))


def case_values(key):
    m = _conv_matrix(key)
    nh = m.num_haplotypes
    lay = pchk.Layout.of(m)
    payload = np.arange(lay.n_bits, dtype=np.float64) * 3.0 + 1.0           # (distinct: a misplaced value cannot hide)
    lib = ecb.load()

    def call(v):
        tot = C.c_uint64(0xDEAD)
        rc = lib.ecb_csr_to_hapcsc_values_device(0, m.num_reads, T, nh, _P(v["ip"]), _P(v["ix"]), _P(v["da"]), _P(v["values"]), _P(v["cp"]), _P(v["ci"]),
                                                 _P(v["cd"]), C.byref(tot))
        return rc, tot.value

    def verify(out, tot):
        assert tot == lay.n_bits
        assert np.array_equal(out["cp"], lay.csc_indptr) and np.array_equal(out["ci"], lay.csc_indices)
        assert out["cd"].tobytes() == lay.to_csc(payload).tobytes()
    return Case(_csr_ins(m, n=False) + [("values", payload, np.float64)],
                [("cp", (nh, T + 1), np.int32), ("ci", (lay.n_bits,), np.int32), ("cd", (lay.n_bits,), np.float64)], call, verify,
                bad=("ip", _falling(m.indptrA), CONTRACT))


POST_NAMES = ["ip", "ix", "da", "scale", "theta", "gene", "post", "bit_ptr", "mass"]
VALUE_NAMES = ["ip", "ix", "da", "values", "cp", "ci", "cd"]
MODELS = (4, 1, 2, 3)
#: every residue of nnz(A) modulo 4 under the four placements of all arrays, for every model; each array alone off 16 bytes at one of them
POST_PLACED = [(model, k, p) for model in MODELS for k in (0, 1, 2, 3) for p in ("control", "all4", "all8", "all12")] + \
              [(model, 1, "one:" + n) for model in MODELS for n in POST_NAMES]
VALUE_PLACED = [(k, p) for k in (0, 1, 2, 3, "h31") for p in ["control", "all4", "all8", "all12"] + ["one:" + n for n in VALUE_NAMES]]


def _case(model, key):
    return _cached(("post_case", model, key), lambda: case_posterior(key, model))


@pytest.mark.parametrize("model,key,placement", POST_PLACED, ids=["m%d-%s-%s" % c for c in POST_PLACED])
def test_the_posterior_entry_point_on_offset_guarded_views(model, key, placement):
    case = _case(model, key)
    assert case.names == POST_NAMES
    slab, v = _place(case, placement)
    if placement != "control":
        assert any(t.data_ptr() % 16 for t in v.values())
    _good_call(case, slab, v)


@pytest.mark.parametrize("key,placement", VALUE_PLACED, ids=["%s-%s" % c for c in VALUE_PLACED])
def test_the_value_carrying_transposition_on_offset_guarded_views(key, placement):
    case = _cached(("values_case", key), lambda: case_values(key))
    assert case.names == VALUE_NAMES
    slab, v = _place(case, placement)
    if placement != "control":
        assert any(t.data_ptr() % 16 for t in v.values())
    _good_call(case, slab, v)


@pytest.mark.parametrize("entry", ["posterior-m4", "posterior-m1", "posterior-m2", "posterior-m3", "values"])
def test_a_refused_call_on_offset_views_leaves_the_outputs_and_the_guards_alone(entry):
    import torch
    case = _cached(("values_case", 1), lambda: case_values(1)) if entry == "values" else _case(int(entry[-1]), 1)
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
