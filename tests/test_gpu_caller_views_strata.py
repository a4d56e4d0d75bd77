"""``ecb_best_strata_device`` on caller memory as a caller has it: the three inputs and the two outputs as offset, guarded views of one
larger tensor (``tests/caller_views.py``), at every residue of the address modulo 16 that a 4-byte type allows -- the entry point asks
for 4-byte alignment only, and reads and writes a vector of four records where a pointer happens to be 16-byte aligned.  After every
call: the return code, both outputs and the counts against the checker (``tests/strata_checker.py``), and ``Slab.check()`` empty: no
guard byte touched on either side of any array, no input changed -- after a good call, an in-place one and a refused one."""
import ctypes as C

import numpy as np
import pytest

from alntools_amd import ecb, ecb_strata as es

import strata_checker as sk
from caller_views import MARGIN, Slab
from test_gpu_best_strata import FAIL, short_reads
from test_gpu_caller_views import CONTRACT, _P, _cached
from test_strata_constants import G, W

pytestmark = pytest.mark.gpu
N_REC = 2 * G + W + 3                  # three workgroups, the last one a wave and three records: a ragged vector at the end
RES = (0, 4, 8, 12)


def _input():
    rng = np.random.default_rng(23)
    rid, hf, sc = short_reads(rng, N_REC, heads=[W, G, 2 * G])
    rid[W - 40:W + 300] = rid[W - 40]                       # a read over two wave boundaries
    rid[W + 300:] = (rid[W + 300:].astype(np.int64) - (int(rid[W + 300]) - int(rid[W - 40]) - 1)).astype(np.uint32)
    hf[W + 300] = 0
    assert sk.breach(rid, hf) is None
    bad = rid.copy()
    bad[N_REC // 2:] += np.uint32(3)
    return rid, hf, sc, sk.best_strata(rid, hf, sc), bad


def _place(res, extra=()):
    rid, hf, sc, want, bad = _cached("strata_input", _input)
    slab = Slab("cuda", nbytes=(6 + len(extra)) * (4 * N_REC + 2 * MARGIN + 16))
    v = {"rid": slab.place("rid", rid, np.uint32, res[0], "in"), "hf": slab.place("hf", hf, np.uint32, res[1], "in"),
         "sc": slab.place("sc", sc, np.int32, res[2], "in")}
    for name, a in extra:
        v[name] = slab.place(name, a, np.uint32, res[0], "in")
    v["out_rid"] = slab.place("out_rid", (N_REC,), np.uint32, res[3], "out")
    v["out_hf"] = slab.place("out_hf", (N_REC,), np.uint32, res[4], "out")
    return slab, v


def _call(v, rid="rid", out_rid="out_rid", out_hf="out_hf", hf="hf"):
    counts = (C.c_uint64 * 4)(*[7] * 4)
    rc = es.load().ecb_best_strata_device(0, _P(v[rid]), _P(v[hf]), _P(v["sc"]), N_REC, 0, _P(v[out_rid]), _P(v[out_hf]), counts)
    return rc, tuple(counts)


def _good_call(slab, v):
    import torch
    want = _cached("strata_input", _input)[3]
    rc, counts = _call(v)
    torch.cuda.synchronize()
    assert rc == 0, (rc, ecb.load().ecb_last_error(None))
    host = slab.host()
    assert counts == want[2]
    assert np.array_equal(slab.room("out_rid", host).view(np.uint32), want[0]) and np.array_equal(slab.room("out_hf", host).view(np.uint32), want[1])
    assert slab.check(host) == []


PLACED = [(0, 0, 0, 0, 0)] + [(a, (a + 4) % 16, (a + 8) % 16, b, (b + 12) % 16) for a in RES for b in RES] + \
    [tuple(r if k == j else 0 for k in range(5)) for j in range(5) for r in RES[1:]]


@pytest.mark.parametrize("res", PLACED, ids=["rid%d-hf%d-sc%d-outrid%d-outhf%d" % p for p in PLACED])
def test_the_best_strata_entry_point_on_offset_guarded_views(res):
    slab, v = _place(res)
    assert tuple(v[k].data_ptr() % 16 for k in ("rid", "hf", "sc", "out_rid", "out_hf")) == res
    _good_call(slab, v)


@pytest.mark.parametrize("res", [(0, 0, 0, 0, 0), (4, 8, 12, 0, 0), (12, 4, 0, 0, 0)], ids=["aligned", "4-8-12", "12-4-0"])
def test_in_place_on_offset_views(res):
    import torch
    rid, hf, sc, want, bad = _cached("strata_input", _input)
    slab = Slab("cuda", nbytes=4 * (4 * N_REC + 2 * MARGIN + 16))
    v = {"rid": slab.place("rid", rid, np.uint32, res[0], "in"), "hf": slab.place("hf", hf, np.uint32, res[1], "in"),
         "sc": slab.place("sc", sc, np.int32, res[2], "in")}
    rc, counts = _call(v, out_rid="rid", out_hf="hf")
    torch.cuda.synchronize()
    assert rc == 0 and counts == want[2], (rc, ecb.load().ecb_last_error(None))
    host = slab.host()
    assert np.array_equal(slab.room("rid", host).view(np.uint32), want[0]) and np.array_equal(slab.room("hf", host).view(np.uint32), want[1])
    assert [f for f in slab.check(host) if f.side != "input changed"] == []
    assert {f.name for f in slab.check(host)} <= {"rid", "hf"}                  # (the score is never written)


@pytest.mark.parametrize("res", [(4, 12, 8, 4, 0), (0, 0, 0, 8, 12)], ids=["4-12-8-4-0", "0-0-0-8-12"])
def test_a_refused_call_on_offset_views_leaves_the_outputs_and_the_guards_alone(res):
    import torch
    bad = _cached("strata_input", _input)[4]
    slab, v = _place(res, extra=[("rid~bad", bad)])
    rc, counts = _call(v, rid="rid~bad")
    torch.cuda.synchronize()
    assert rc == CONTRACT and counts == (7,) * 4, (rc, ecb.load().ecb_last_error(None))
    assert b"strata: record %d: read_id steps by more than 1" % (N_REC // 2) in ecb.load().ecb_last_error(None)
    host = slab.host()
    assert slab.untouched("out_rid", host) and slab.untouched("out_hf", host)
    assert slab.check(host) == []
    # an output that overlaps an input by one record, and one that is another input: refused, nothing written
    n4 = N_REC - 1
    rc = es.load().ecb_best_strata_device(0, _P(v["rid"]), _P(v["hf"]), _P(v["sc"]), n4, 0, _P(v["rid"][1:]), _P(v["out_hf"]), (C.c_uint64 * 4)())
    assert rc == -1 and b"overlaps" in ecb.load().ecb_last_error(None)
    rc, _ = _call(v, out_rid="hf")
    assert rc == -1 and b"overlaps" in ecb.load().ecb_last_error(None)
    assert slab.check() == [] and slab.untouched("out_rid") and slab.untouched("out_hf")
    _good_call(slab, v)
