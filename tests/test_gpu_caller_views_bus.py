"""bus2ec's device entry point (``ecb_bus_molecules_device``; its host twin takes no device memory) on caller memory as a caller has it:
offset, guarded views of one larger tensor (``tests/caller_views.py``), in the manner of ``test_gpu_caller_views_components.py`` -- every
residue modulo 16 the element types allow (the records are bytes: residues 1, 7 and 15 too), all arrays at once and each alone.  After every
call: the return code, every output against the checker (``tests/bus_checker.py``), nothing written behind what ``out_sizes`` reports, and
``Slab.check()`` empty: no guard byte touched on either side of any array, no input changed -- after a good call and after a refused one."""
import ctypes as C

import numpy as np
import pytest

from alntools_amd import ecb, ecb_bus

import bus_checker as bc
from caller_views import FILL
from test_gpu_caller_views import CONTRACT, Case, _P, _cached, _good_call, _place

pytestmark = pytest.mark.gpu
T, H = 90, 3
TCOL, THAP = (np.arange(T) // H).astype(np.uint32), (np.arange(T) % H).astype(np.uint32)
OUTS = ["ob", "oipa", "oixa", "odaa", "oipn", "oixn", "odn", "orl"]
N_REC = 2 * 1024 + 37


def _input():
    rng = np.random.default_rng(17)
    core = [3, 40, 77]
    lines = [sorted(set(rng.choice(T, size=int(rng.integers(1, 9)), replace=False).tolist()) | set(core[:int(rng.integers(0, 4))])) for _ in range(50)]
    cells = rng.choice(1 << 24, size=9, replace=False).astype(np.uint64)
    rec = bc.records(cells[rng.integers(0, 9, size=N_REC)], rng.integers(0, 150, size=N_REC).astype(np.uint64), rng.integers(0, 50, size=N_REC),
                     rng.integers(0, 4, size=N_REC))
    return rec, lines, np.sort(cells)


def case_bus(key):
    rec, lines, cells = _cached("bus_input", _input)
    no_umi, keep = bool(key & 2), (cells[[0, 2, 3, 5, 8]] if key & 1 else None)
    ptr, ids = bc.csr_lines(lines)
    want = bc.molecules(rec, lines, TCOL, THAP, keep=keep, no_umi=no_umi)
    caps = (N_REC if keep is None else len(keep), N_REC, ecb_bus.a_capacity(rec, ptr), N_REC)
    lib = ecb_bus.load()

    def call(v):
        sizes = (C.c_uint64 * 8)(*[7] * 8)
        rc = lib.ecb_bus_molecules_device(0, _P(v["rec"]), N_REC, 12, 8, ecb_bus.NO_UMI if no_umi else 0, len(lines), len(ids), _P(v["ptr"]), _P(v["ids"]),
                                          T, _P(v["tcol"]), _P(v["thap"]), T // H, H, _P(v["keep"]) if keep is not None else None,
                                          0 if keep is None else len(keep), *caps, *([_P(v[n]) for n in OUTS] + [sizes]))
        return rc, tuple(sizes)

    def verify(out, sizes):
        assert sizes == want.sizes
        cells_n, rows, nnz_a, nnz_n = sizes[:4]
        exp = [np.array(want.barcodes, dtype=np.uint64)] + list(bc.csr(want.rows)) + list(bc.csc(want.N, cells_n)) + [np.array(want.row_line, dtype=np.int32)]
        for name, e in zip(OUTS, exp):
            got = out[name].reshape(-1)
            assert np.array_equal(got[:len(e)], e), name
            assert (got[len(e):].view(np.uint8) == FILL).all(), name + ": written behind the result"
        assert len(exp[1]) == rows + 1 and len(exp[2]) == nnz_a and len(exp[5]) == nnz_n
    ins = [("rec", rec.reshape(-1), np.uint8), ("ptr", ptr, np.uint32), ("ids", ids, np.uint32), ("tcol", TCOL, np.uint32), ("thap", THAP, np.uint32)]
    if keep is not None:
        ins.append(("keep", keep, np.uint64))
    outs = [("ob", (caps[0],), np.uint64), ("oipa", (caps[1] + 1,), np.int32), ("oixa", (caps[2],), np.int32), ("odaa", (caps[2],), np.int32),
            ("oipn", (caps[0] + 1,), np.int32), ("oixn", (caps[3],), np.int32), ("odn", (caps[3],), np.int32), ("orl", (caps[1],), np.int32)]
    bad = rec.copy().reshape(-1, 32)
    bad[N_REC // 2, 16:20] = np.array([len(lines)], dtype="<i4").view(np.uint8)
    return Case(ins, outs, call, verify, bad=("rec", bad.reshape(-1), CONTRACT))


def _names(key):
    return ["rec", "ptr", "ids", "tcol", "thap"] + (["keep"] if key & 1 else []) + OUTS


ALL = ["control", "all4", "all8", "all12"]
PLACED = [(k, p) for k in (0, 1, 2, 3) for p in ALL] + [(1, "one:" + n) for n in _names(1)]


@pytest.mark.parametrize("key,placement", PLACED, ids=["%s-%s" % c for c in PLACED])
def test_the_bus_entry_point_on_offset_guarded_views(key, placement):
    case = _cached(("bus_case", key), lambda: case_bus(key))
    assert case.names == _names(key)
    slab, v = _place(case, placement)
    if placement != "control":
        assert any(t.data_ptr() % 16 for t in v.values())
    if placement.startswith("all"):
        assert v["rec"].data_ptr() % 2 == 1                       # (the records at an odd address)
    _good_call(case, slab, v)


@pytest.mark.parametrize("key", [1, 2])
def test_a_refused_call_on_offset_views_leaves_the_outputs_and_the_guards_alone(key):
    import torch
    case = _cached(("bus_case", key), lambda: case_bus(key))
    name, bad, code = case.bad
    slab, v = _place(case, "all4", extra=[(name + "~bad", bad, np.uint8)])
    rc, sizes = case.call(dict(v, **{name: v[name + "~bad"]}))
    torch.cuda.synchronize()
    assert rc == code and sizes == (7,) * 8, (rc, ecb.load().ecb_last_error(None))
    assert b"bus: record %d: " % (N_REC // 2) in ecb.load().ecb_last_error(None)
    host = slab.host()
    for out, _, _ in case.outs:
        assert slab.untouched(out, host), out
    assert slab.check(host) == []
    _good_call(case, slab, v)
