"""``ecb_collapse_umis_device`` on caller memory as a caller has it: the four inputs and the four outputs as offset, guarded views of one
larger tensor (``tests/caller_views.py``), at every residue of the address modulo 16 that their element types allow -- the entry point
asks for the element's alignment only.  After every call: the return code, the outputs and the counts against the checker
(``tests/umi_checker.py``), and ``Slab.check()`` empty: no guard byte touched on either side of any array, no input changed -- after a
good call and after a refused one.  The outputs have their documented room, n records and n_reads first reads; what lies behind the
records and molecules that came out stays as it was."""
import ctypes as C

import numpy as np
import pytest

from alntools_amd import ecb, ecb_umi as eu

import umi_checker as uc
from caller_views import FILL, MARGIN, Slab
from test_gpu_caller_views import CONTRACT, _P, _cached
from test_gpu_collapse_umis import N_HAPS, N_LOCI, molecule_stream, build
from test_umi_constants import G, W

pytestmark = pytest.mark.gpu
RES4, RES8 = (0, 4, 8, 12), (0, 8)
NAMES = ("rid", "loc", "hf", "key", "out_rid", "out_loc", "out_hf", "out_first")


def _input():
    rng = np.random.default_rng(29)
    reads, keys = molecule_stream(rng, [1, 2, 3, W + 1, 1, 1, 2] * 3 + [G + 3, 1, 2], "shuffled")
    rid, loc, hf = build(reads, first_id=3, lead=2)
    keys = np.array(keys, dtype=np.uint64)
    assert uc.breach(rid, loc, hf, len(keys), N_LOCI, N_HAPS) is None and len(rid) > 2 * G
    bad = rid.copy()
    bad[len(rid) // 2:] += np.uint32(3)
    return rid, loc, hf, keys, uc.collapse(rid, loc, hf, keys), bad


def _place(res, extra=()):
    rid, loc, hf, keys, want, bad = _cached("umi_input", _input)
    n, nr = len(rid), len(keys)
    slab = Slab("cuda", nbytes=(8 + len(extra)) * (4 * n + 2 * MARGIN + 16) + 8 * nr)
    v = {"rid": slab.place("rid", rid, np.uint32, res[0], "in"), "loc": slab.place("loc", loc, np.uint32, res[1], "in"),
         "hf": slab.place("hf", hf, np.uint32, res[2], "in"), "key": slab.place("key", keys, np.uint64, res[3], "in")}
    for name, a in extra:
        v[name] = slab.place(name, a, np.uint32, res[0], "in")
    for k, name in enumerate(("out_rid", "out_loc", "out_hf")):
        v[name] = slab.place(name, (n,), np.uint32, res[4 + k], "out")
    v["out_first"] = slab.place("out_first", (nr,), np.uint32, res[7], "out")
    return slab, v


def _call(v, rid="rid", out_rid="out_rid", out_first="out_first", n_reads=None):
    keys = _cached("umi_input", _input)[3]
    counts = (C.c_uint64 * 6)(*[7] * 6)
    rc = eu.load().ecb_collapse_umis_device(0, _P(v[rid]), _P(v["loc"]), _P(v["hf"]), _P(v["key"]), v["rid"].numel(), len(keys) if n_reads is None else n_reads,
                                            N_LOCI, N_HAPS, _P(v[out_rid]), _P(v["out_loc"]), _P(v["out_hf"]), _P(v[out_first]), counts)
    return rc, tuple(counts)


def _good_call(slab, v):
    import torch
    want = _cached("umi_input", _input)[4]
    rc, counts = _call(v)
    torch.cuda.synchronize()
    assert rc == 0, (rc, ecb.load().ecb_last_error(None))
    host = slab.host()
    assert counts == want[4]
    for k, name in enumerate(("out_rid", "out_loc", "out_hf", "out_first")):
        room = slab.room(name, host).view(np.uint32)
        m = len(want[k])
        assert np.array_equal(room[:m], want[k]), name
        assert (room[m:].view(np.uint8) == FILL).all(), name + ": written behind what came out"
    assert slab.check(host) == []


PLACED = [(0,) * 8] + [(a, (a + 4) % 16, (a + 8) % 16, k, b, (b + 12) % 16, (b + 8) % 16, (a + b) % 16) for a in RES4 for b in RES4 for k in RES8 if (a + b) % 8 == 0 or k] + \
    [tuple(r if k == j else 0 for k in range(8)) for j in range(8) for r in (RES8[1:] if j == 3 else RES4[1:])]


@pytest.mark.parametrize("res", PLACED, ids=["-".join("%s%d" % (n, r) for n, r in zip(NAMES, p)) for p in PLACED])
def test_the_collapse_entry_point_on_offset_guarded_views(res):
    slab, v = _place(res)
    assert tuple(v[k].data_ptr() % 16 for k in NAMES) == res
    _good_call(slab, v)


@pytest.mark.parametrize("res", [(4, 12, 8, 8, 4, 0, 12, 8), (0, 0, 0, 0, 8, 12, 4, 4)], ids=["4-12-8-8-4-0-12-8", "0-0-0-0-8-12-4-4"])
def test_a_refused_call_on_offset_views_leaves_the_outputs_and_the_guards_alone(res):
    import torch
    rid, loc, hf, keys, want, bad = _cached("umi_input", _input)
    slab, v = _place(res, extra=[("rid~bad", bad)])
    outs = ("out_rid", "out_loc", "out_hf", "out_first")
    rc, counts = _call(v, rid="rid~bad")
    torch.cuda.synchronize()
    assert rc == CONTRACT and counts == (7,) * 6, (rc, ecb.load().ecb_last_error(None))
    assert b"umi: record %d: read_id steps by more than 1" % (len(rid) // 2) in ecb.load().ecb_last_error(None)
    rc, counts = _call(v, n_reads=len(keys) - 1)              # one read more than the caller says: nothing of its key or first read is touched
    torch.cuda.synchronize()
    assert rc == CONTRACT and counts == (7,) * 6 and b"the stream holds %d reads, n_reads is %d" % (len(keys), len(keys) - 1) in ecb.load().ecb_last_error(None)
    host = slab.host()
    assert all(slab.untouched(o, host) for o in outs) and slab.check(host) == []
    # an output that overlaps an input by one record, one that is another input, one that is another output: refused, nothing written
    lib = eu.load()
    n = len(rid) - 1
    rc = lib.ecb_collapse_umis_device(0, _P(v["rid"]), _P(v["loc"]), _P(v["hf"]), _P(v["key"]), n, len(keys), N_LOCI, N_HAPS, _P(v["rid"][1:]), _P(v["out_loc"]),
                                      _P(v["out_hf"]), _P(v["out_first"]), (C.c_uint64 * 6)())
    assert rc == -1 and b"overlaps" in lib.ecb_last_error(None)
    for kw in (dict(out_rid="hf"), dict(out_first="out_hf"), dict(out_rid="key")):
        rc, _ = _call(v, **kw)
        assert rc == -1 and b"overlaps" in lib.ecb_last_error(None), kw
    # a key array that is not 8-byte aligned
    rc = lib.ecb_collapse_umis_device(0, _P(v["rid"]), _P(v["loc"]), _P(v["hf"]), _P(v["rid"][1:]) if v["rid"].data_ptr() % 8 == 0 else _P(v["rid"]), n, len(keys),
                                      N_LOCI, N_HAPS, _P(v["out_rid"]), _P(v["out_loc"]), _P(v["out_hf"]), _P(v["out_first"]), (C.c_uint64 * 6)())
    assert rc == -1 and b"aligned" in lib.ecb_last_error(None)
    assert slab.check() == [] and all(slab.untouched(o) for o in outs)
    _good_call(slab, v)
