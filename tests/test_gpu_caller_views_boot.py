"""ecboot's device entry points (``ecb_resample_device``, ``ecb_quantify_bootstrap_device``; their host twins take no device memory) on
caller memory as a caller has it: offset, guarded views of one larger tensor (``tests/caller_views.py``), in the manner and with the
matrices of ``test_gpu_caller_views.py`` -- every residue modulo 16 the element types allow, all arrays at once and each alone.  After
every call: the return code, the result against the checker (the replicates byte for byte; the bootstrap's replicates byte for byte what
``ecb.quantify_cells`` gives on the checker's resampled N, its moments bit for bit the same call on aligned tensors), and ``Slab.check()``
empty: no guard byte touched on either side of any array, no input changed."""
import ctypes as C

import numpy as np
import pytest

from alntools_amd import ecb, ecb_boot

import boot_checker as bc
from caller_views import _torch_dtype
from test_gpu_caller_views import CONTRACT, H, S, T, Case, _P, _cached, _csr_ins, _good_call, _matrix, _place

pytestmark = pytest.mark.gpu
SEED, B0, B = 9, 2, 3
ITERS, TOL = 12, 1e-4


def _replicates(key, sample):
    m = _matrix(key, 1)
    return _cached(("boot_reps", key, sample), lambda: bc.resample(bc.weights(m.num_reads, m.indptrN, m.indicesN, m.dataN, sample), SEED, B0, B))


def case_resample(key):
    m = _matrix(key, 1)
    sample = None if key % 2 else 4
    ptr, ec, cnt, _ = _replicates(key, sample)
    lib = ecb_boot.load()

    def call(v):
        n = C.c_uint64(0xDEAD)
        rc = lib.ecb_resample_device(0, m.num_reads, S, len(m.indicesN), _P(v["pn"]), _P(v["xn"]), _P(v["dn"]), -1 if sample is None else sample, SEED, B0, B,
                                     _P(v["rp"]), _P(v["re"]), _P(v["rc"]), len(ec), C.byref(n))
        return rc, n.value

    def verify(out, n):
        assert n == len(ec) and out["rp"].tobytes() == ptr.tobytes() and out["re"].tobytes() == ec.tobytes() and out["rc"].tobytes() == cnt.tobytes()
    neg = m.dataN.copy()
    neg[len(neg) // 2] = -3
    return Case(_csr_ins(m)[3:], [("rp", (B + 1,), np.int32), ("re", (len(ec),), np.int32), ("rc", (len(ec),), np.int32)], call, verify,
                bad=("dn", neg, CONTRACT))


BOOT_OUTS = [("mean", (H, T), np.float64), ("sd", (H, T), np.float64), ("tm", (T,), np.float64), ("ts", (T,), np.float64), ("reps", (B, H, T), np.float64),
             ("it", (B,), np.uint32), ("dl", (B,), np.float64), ("ex", (B,), np.int64), ("cv", (B,), np.uint8)]


def _bootstrap(m, v, scale="scale"):
    rc = ecb_boot.load().ecb_quantify_bootstrap_device(
        0, m.num_reads, T, H, len(m.indicesA), _P(v["ip"]), _P(v["ix"]), _P(v["da"]), S, len(m.indicesN), _P(v["pn"]), _P(v["xn"]), _P(v["dn"]), -1,
        _P(v[scale]), ITERS, TOL, 0, 0, None, 4, SEED, B, *[_P(v[n]) for n, _, _ in BOOT_OUTS])
    return rc, None


def case_bootstrap(key):
    import torch
    m = _matrix(key, 1)
    scale = 1.0 / np.random.default_rng(70 + key).integers(1, 3000, size=(H, T))
    ins = _csr_ins(m) + [("scale", scale, np.float64)]
    ptr, ec, cnt, _ = _cached(("boot_reps0", key), lambda: bc.resample(bc.weights(m.num_reads, m.indptrN, m.indicesN, m.dataN), SEED, 0, B))
    cp, sl, th, info = ecb.quantify_cells(m.indptrA, m.indicesA, m.dataA, T, H, ptr, ec, cnt, scale=scale, max_iters=ITERS, tol=TOL)
    want = bc.scatter(cp, sl, th, T, H)

    def aligned():
        v = {n: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda() for n, a, dt in ins}
        for n, shape, dt in BOOT_OUTS:
            v[n] = torch.zeros(shape, dtype=_torch_dtype(np.dtype(dt)), device="cuda")
        assert all(t.data_ptr() % 16 == 0 for t in v.values())
        assert _bootstrap(m, v)[0] == 0
        torch.cuda.synchronize()
        return {n: v[n].cpu().numpy().tobytes() for n, _, _ in BOOT_OUTS}
    plain = _cached(("boot_aligned", key), aligned)

    def verify(out, _):
        assert out["reps"].tobytes() == want.tobytes()
        assert np.array_equal(out["it"], info["n_iter"]) and np.array_equal(out["dl"], info["delta"]) and np.array_equal(out["ex"], info["explained"])
        assert np.array_equal(out["cv"] != 0, info["converged"])
        assert all(out[n].tobytes() == plain[n] for n, _, _ in BOOT_OUTS)
        # (the moments against the checker's loop, within the bound test_gpu_ecboot.py derives: 3 B 2^-52 of the entry's largest replicate)
        assert (np.abs(out["mean"] - bc.welford(want)[0]) <= 3 * B * 2.0 ** -52 * want.max(axis=0)).all() and out["sd"].max() > 0
    bad = scale.copy()
    bad[1, T // 2] = np.nan
    return Case(ins, BOOT_OUTS, lambda v: _bootstrap(m, v), verify, bad=("scale", bad, CONTRACT))


RESAMPLE_NAMES = ["pn", "xn", "dn", "rp", "re", "rc"]
BOOT_NAMES = ["ip", "ix", "da", "pn", "xn", "dn", "scale"] + [n for n, _, _ in BOOT_OUTS]
ALL = ["control", "all4", "all8", "all12"]
RESAMPLE_PLACED = [(k, p) for k in (0, 1, 2, 3) for p in ALL] + [(1, "one:" + n) for n in RESAMPLE_NAMES]
BOOT_PLACED = [(1, p) for p in ALL + ["one:" + n for n in BOOT_NAMES]]


@pytest.mark.parametrize("key,placement", RESAMPLE_PLACED, ids=["%s-%s" % c for c in RESAMPLE_PLACED])
def test_the_resampling_entry_point_on_offset_guarded_views(key, placement):
    case = _cached(("resample_case", key), lambda: case_resample(key))
    assert case.names == RESAMPLE_NAMES
    slab, v = _place(case, placement)
    if placement != "control":
        assert any(t.data_ptr() % 16 for t in v.values())
    _good_call(case, slab, v)


@pytest.mark.parametrize("key,placement", BOOT_PLACED, ids=["%s-%s" % c for c in BOOT_PLACED])
def test_the_bootstrap_entry_point_on_offset_guarded_views(key, placement):
    case = _cached(("bootstrap_case", key), lambda: case_bootstrap(key))
    assert case.names == BOOT_NAMES
    slab, v = _place(case, placement)
    if placement != "control":
        assert any(t.data_ptr() % 16 for t in v.values())
    _good_call(case, slab, v)


@pytest.mark.parametrize("entry", ["resample", "bootstrap"])
def test_a_refused_call_on_offset_views_leaves_the_outputs_and_the_guards_alone(entry):
    import torch
    case = _cached((entry + "_case", 1), lambda: (case_resample if entry == "resample" else case_bootstrap)(1))
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
