"""``ecb_downsample_device`` on caller memory as a caller has it: the four inputs and the three outputs as offset, guarded views of one
larger tensor (``tests/caller_views.py``), at every residue of the address modulo 16 that their element types allow -- the entry point
asks for the element's alignment only.  After every call: the return code and the outputs against the checker
(``tests/downsample_checker.py``), and ``Slab.check()`` empty: no guard byte touched on either side of any array, no input changed --
after a good call and after a refused one."""
import numpy as np
import pytest

from alntools_amd import ecb, ecb_downsample as ed

import downsample_checker as dc
from caller_views import MARGIN, Slab
from test_gpu_caller_views import ARG, CONTRACT, _P, _cached
from test_gpu_ecdownsample import _mixed

pytestmark = pytest.mark.gpu
RES4, RES8 = (0, 4, 8, 12), (0, 8)
NAMES = ("pn", "xn", "dn", "tg", "out", "tin", "tout")
SEED = 33


def _input():
    ptr, ec, cnt, E, Ms = _mixed()
    target = Ms // 2
    target[1], target[6] = -1, 0                         # a copied column, an emptied one, small and large ones thinned
    bad = np.array(cnt).copy()
    bad[len(bad) // 3] = -1
    return ptr, ec, cnt, E, target, dc.downsample(ptr, ec, cnt, E, target, SEED), bad


def _place(res, extra=()):
    ptr, ec, cnt, E, target, want, bad = _cached("downsample_input", _input)
    nnz, S = len(ec), len(target)
    slab = Slab("cuda", nbytes=(4 + len(extra)) * (4 * nnz + 2 * MARGIN + 16) + 4 * (8 * S + 2 * MARGIN + 16))
    v = {"pn": slab.place("pn", ptr, np.int32, res[0], "in"), "xn": slab.place("xn", ec, np.int32, res[1], "in"),
         "dn": slab.place("dn", cnt, np.int32, res[2], "in"), "tg": slab.place("tg", target, np.int64, res[3], "in")}
    for name, a in extra:
        v[name] = slab.place(name, a, np.int32, res[2], "in")
    v["out"] = slab.place("out", (nnz,), np.int32, res[4], "out")
    v["tin"] = slab.place("tin", (S,), np.int64, res[5], "out")
    v["tout"] = slab.place("tout", (S,), np.int64, res[6], "out")
    return slab, v


def _call(v, dn="dn", out="out", tin="tin", tout="tout"):
    E = _cached("downsample_input", _input)[3]
    return ed.load().ecb_downsample_device(0, E, v["tg"].numel(), v["xn"].numel(), _P(v["pn"]), _P(v["xn"]), _P(v[dn]), _P(v["tg"]), SEED,
                                           _P(v[out]), _P(v[tin]) if tin else None, _P(v[tout]) if tout else None)


def _good_call(slab, v):
    import torch
    want = _cached("downsample_input", _input)[5]
    rc = _call(v)
    torch.cuda.synchronize()
    assert rc == 0, (rc, ecb.load().ecb_last_error(None))
    host = slab.host()
    assert np.array_equal(slab.room("out", host).view(np.int32), want[0])
    assert np.array_equal(slab.room("tin", host).view(np.int64), want[1]) and np.array_equal(slab.room("tout", host).view(np.int64), want[2])
    assert slab.check(host) == []


PLACED = [(0,) * 7] + [(a, (a + 4) % 16, (a + 8) % 16, k, b, (k + 8) % 16, k) for a in RES4 for b in RES4 for k in RES8 if (a + b) % 8 == 0 or k] + \
    [tuple(r if k == j else 0 for k in range(7)) for j in range(7) for r in (RES8[1:] if j in (3, 5, 6) else RES4[1:])]


@pytest.mark.parametrize("res", PLACED, ids=["-".join("%s%d" % (n, r) for n, r in zip(NAMES, p)) for p in PLACED])
def test_the_downsample_entry_point_on_offset_guarded_views(res):
    slab, v = _place(res)
    assert tuple(v[k].data_ptr() % 16 for k in NAMES) == res
    _good_call(slab, v)


@pytest.mark.parametrize("res", [(4, 12, 8, 8, 4, 0, 8), (0, 0, 0, 0, 12, 8, 8)], ids=["4-12-8-8-4-0-8", "0-0-0-0-12-8-8"])
def test_a_refused_call_on_offset_views_leaves_the_outputs_and_the_guards_alone(res):
    import torch
    slab, v = _place(res, extra=[("dn~bad", _cached("downsample_input", _input)[6])])
    outs = ("out", "tin", "tout")
    lib = ed.load()
    rc = _call(v, dn="dn~bad")
    torch.cuda.synchronize()
    assert rc == CONTRACT and b"a negative count" in lib.ecb_last_error(None)
    host = slab.host()
    assert all(slab.untouched(o, host) for o in outs) and slab.check(host) == []
    # an output that is an input, an output that is another output, an output one entry into an input: refused, nothing written
    for kw in (dict(out="dn"), dict(out="xn"), dict(tin="tg"), dict(tout="tin")):
        assert _call(v, **kw) == ARG and b"overlaps" in lib.ecb_last_error(None), kw
    rc = lib.ecb_downsample_device(0, _cached("downsample_input", _input)[3], v["tg"].numel(), v["xn"].numel() - 1, _P(v["pn"]), _P(v["xn"]), _P(v["dn"]),
                                   _P(v["tg"]), SEED, _P(v["dn"][1:]), None, None)
    assert rc == ARG and b"overlaps" in lib.ecb_last_error(None)
    # a target array that is not 8-byte aligned
    odd = v["dn"] if v["dn"].data_ptr() % 8 else v["dn"][1:]
    rc = lib.ecb_downsample_device(0, _cached("downsample_input", _input)[3], v["tg"].numel(), v["xn"].numel(), _P(v["pn"]), _P(v["xn"]), _P(v["dn"]),
                                   _P(odd), SEED, _P(v["out"]), None, None)
    assert rc == ARG and b"aligned" in lib.ecb_last_error(None)
    assert slab.check() == [] and all(slab.untouched(o) for o in outs)
    _good_call(slab, v)
