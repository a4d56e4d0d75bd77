"""ecclusters' device entry point (``ecb_components_device``; its host twin takes no device memory) on caller memory as a caller has it:
offset, guarded views of one larger tensor (``tests/caller_views.py``), in the manner and with the matrices of
``test_gpu_caller_views.py`` -- every residue modulo 16 the element types allow, all arrays at once and each alone.  After every call: the
return code, every output against the checker (``tests/components_checker.py``), and ``Slab.check()`` empty: no guard byte touched on either
side of any array, no input changed -- after a good call and after a refused one."""
import ctypes as C

import numpy as np
import pytest

from alntools_amd import ecb, ecb_components

import components_checker as cc
from test_gpu_caller_views import CONTRACT, H, S, T, Case, _P, _cached, _csr_ins, _falling, _good_call, _matrix, _place

pytestmark = pytest.mark.gpu
OUTS = ["ol", "oe", "cl", "ce", "cr"]


def case_components(key):
    zeros = key % 2
    m = _matrix(key, zeros)
    sample = None if key < 2 else 4
    mc = 1 if key < 3 else 30
    want = cc.components(m.indptrA, m.indicesA, m.dataA, T, H, m.indptrN, m.indicesN, m.dataN, sample=sample, min_count=mc)
    lib = ecb_components.load()

    def call(v):
        sizes = (C.c_uint64 * 4)(7, 7, 7, 7)
        rc = lib.ecb_components_device(0, m.num_reads, T, H, len(m.indicesA), _P(v["ip"]), _P(v["ix"]), _P(v["da"]), S, len(m.indicesN), _P(v["pn"]),
                                       _P(v["xn"]), _P(v["dn"]), -1 if sample is None else sample, mc, *([_P(v[n]) for n in OUTS] + [sizes]))
        return rc, tuple(sizes)

    def verify(out, sizes):
        n = want[5][0]
        assert sizes == want[5]
        assert np.array_equal(out["ol"], want[0]) and np.array_equal(out["oe"], want[1])
        for name, e in zip(OUTS[2:], want[2:5]):
            assert np.array_equal(out[name][:n], e) and not out[name][n:].any(), name
    outs = [("ol", (T,), np.int32), ("oe", (m.num_reads,), np.int32), ("cl", (T,), np.int32), ("ce", (T,), np.int32), ("cr", (T,), np.int64)]
    return Case(_csr_ins(m), outs, call, verify, bad=("ip", _falling(m.indptrA), CONTRACT))


NAMES = ["ip", "ix", "da", "pn", "xn", "dn"] + OUTS
ALL = ["control", "all4", "all8", "all12"]
PLACED = [(k, p) for k in (0, 1, 2, 3) for p in ALL] + [(1, "one:" + n) for n in NAMES]


@pytest.mark.parametrize("key,placement", PLACED, ids=["%s-%s" % c for c in PLACED])
def test_the_components_entry_point_on_offset_guarded_views(key, placement):
    case = _cached(("components_case", key), lambda: case_components(key))
    assert case.names == NAMES
    slab, v = _place(case, placement)
    if placement != "control":
        assert any(t.data_ptr() % 16 for t in v.values())
    _good_call(case, slab, v)


@pytest.mark.parametrize("which", ["ip", "dn"])
def test_a_refused_call_on_offset_views_leaves_the_outputs_and_the_guards_alone(which):
    import torch
    case = _cached(("components_case", 1), lambda: case_components(1))
    name, bad, code = case.bad
    if which == "dn":
        m = _matrix(1, 1)
        bad = m.dataN.copy()
        bad[len(bad) // 2] = -3
        name = "dn"
    slab, v = _place(case, "all4", extra=[(name + "~bad", bad, np.int32)])
    rc, sizes = case.call(dict(v, **{name: v[name + "~bad"]}))
    torch.cuda.synchronize()
    assert rc == code and sizes == (7, 7, 7, 7), (rc, ecb.load().ecb_last_error(None))
    host = slab.host()
    for out, _, _ in case.outs:
        assert slab.untouched(out, host), out
    assert slab.check(host) == []
    _good_call(case, slab, v)
