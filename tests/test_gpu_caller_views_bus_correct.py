"""Barcode correction's device entry point (``ecb_bus_correct_device``; its host twin takes no device memory) on caller memory as a caller
has it: offset, guarded views of one larger tensor (``tests/caller_views.py``), in the manner of ``test_gpu_caller_views_bus.py``.  The
records, in and out, are bytes and go to every byte residue modulo 16; the whitelist (uint64) to 0 and 8; the status (bytes) wherever the
records go.  After every call: the return code, every output against the checker (``tests/bus_correct_checker.py``), nothing written
behind what ``out_sizes`` reports, and ``Slab.check()`` empty: no guard byte touched on either side of any array, no input changed --
after a good call and after a refused one."""
import ctypes as C

import numpy as np
import pytest

from alntools_amd import ecb, ecb_bus_correct as ebc

import bus_checker as bc
import bus_correct_checker as cc
from caller_views import FILL, MARGIN, Slab
from test_gpu_caller_views import CONTRACT, _P, _cached

pytestmark = pytest.mark.gpu
N_REC = 2 * 1024 + 37
BCLEN = 16


def _input():
    rng = np.random.default_rng(17)
    cells = []
    while len(cells) < 30:
        s = "".join(rng.choice(list(bc.BASES), size=BCLEN))
        if all(cc.distance(s, x) >= 3 for x in cells):
            cells.append(s)
    cells.append(cells[0][:5] + bc.BASES[(bc.BASES.index(cells[0][5]) + 1) % 4] + cells[0][6:])      # (one base from cells[0]: ambiguity is possible)
    white = np.array(sorted(bc.encode(s) for s in cells), dtype=np.uint64)
    seqs = []
    for i in range(N_REC):
        s = cells[int(rng.integers(len(cells)))]
        for _ in range(int(rng.choice(3, p=[0.6, 0.3, 0.1]))):                                        # none, one or two bases changed
            p = int(rng.integers(BCLEN))
            s = s[:p] + bc.BASES[(bc.BASES.index(s[p]) + int(rng.integers(1, 4))) % 4] + s[p + 1:]
        seqs.append(s)
    rec = bc.records(np.array([bc.encode(s) for s in seqs], dtype=np.uint64), rng.integers(0, 1 << 24, size=N_REC).astype(np.uint64),
                     rng.integers(0, 50, size=N_REC), rng.integers(0, 4, size=N_REC), flags=rng.integers(0, 1 << 32, size=N_REC))
    want = cc.correct(rec, BCLEN, white)
    assert all(want[2]) and len(want[1]) < N_REC
    bad = rec.copy()
    bad[N_REC // 2, :8] = np.array([1 << 32], dtype="<u8").view(np.uint8)
    return rec, white, want, bad


def _place(rec_res, out_res, white_res, status_res, extra=()):
    rec, white, want, bad = _cached("bus_correct_input", _input)
    slab = Slab("cuda", nbytes=3 * rec.size + white.size * 8 + N_REC + 8 * (2 * MARGIN + 16))
    v = {"rec": slab.place("rec", rec.reshape(-1), np.uint8, rec_res, "in"), "white": slab.place("white", white, np.uint64, white_res, "in")}
    for name, a in extra:
        v[name] = slab.place(name, a.reshape(-1), np.uint8, rec_res, "in")
    v["out"] = slab.place("out", (N_REC * 32,), np.uint8, out_res, "out")
    v["status"] = slab.place("status", (N_REC,), np.uint8, status_res, "out")
    return slab, v


def _call(v, rec="rec"):
    sizes = (C.c_uint64 * 4)(*[7] * 4)
    rc = ebc.load().ecb_bus_correct_device(0, _P(v[rec]), N_REC, BCLEN, _P(v["white"]), v["white"].numel(), N_REC, _P(v["out"]), _P(v["status"]), sizes)
    return rc, tuple(sizes)


def _good_call(slab, v):
    import torch
    want = _cached("bus_correct_input", _input)[2]
    rc, sizes = _call(v)
    torch.cuda.synchronize()
    assert rc == 0, (rc, ecb.load().ecb_last_error(None))
    host = slab.host()
    assert sizes == want[2]
    out, status = slab.room("out", host), slab.room("status", host)
    kept = want[1].reshape(-1)
    assert np.array_equal(out[:len(kept)], kept) and (out[len(kept):] == FILL).all(), "out: wrong, or written behind the result"
    assert np.array_equal(status, want[0])
    assert slab.check(host) == []


# the records (bytes) at every residue modulo 16, in and out on different ones; the whitelist on both of its two
PLACED = [(0, 0, 0, 0)] + [(r, (r * 7 + 3) % 16, 8 * (r % 2), (r + 5) % 16) for r in range(16)] + [(0, r, 0, 0) for r in range(1, 16)]


@pytest.mark.parametrize("rec_res,out_res,white_res,status_res", PLACED, ids=["rec%d-out%d-white%d-status%d" % p for p in PLACED])
def test_the_bus_correct_entry_point_on_offset_guarded_views(rec_res, out_res, white_res, status_res):
    slab, v = _place(rec_res, out_res, white_res, status_res)
    assert (v["rec"].data_ptr() % 16, v["out"].data_ptr() % 16, v["white"].data_ptr() % 16, v["status"].data_ptr() % 16) == (rec_res, out_res, white_res, status_res)
    _good_call(slab, v)


@pytest.mark.parametrize("res", [1, 12])
def test_a_refused_call_on_offset_views_leaves_the_outputs_and_the_guards_alone(res):
    import torch
    bad = _cached("bus_correct_input", _input)[3]
    slab, v = _place(res, (res + 6) % 16, 8, 3, extra=[("rec~bad", bad)])
    rc, sizes = _call(v, rec="rec~bad")
    torch.cuda.synchronize()
    assert rc == CONTRACT and sizes == (7,) * 4, (rc, ecb.load().ecb_last_error(None))
    assert b"bus: record %d: " % (N_REC // 2) in ecb.load().ecb_last_error(None)
    host = slab.host()
    assert slab.untouched("out", host) and slab.untouched("status", host)
    assert slab.check(host) == []
    _good_call(slab, v)
