"""The lifecycle of an ``ecb_handle`` (``ecb.hip: ecb_handle::Run``, ``Stage``, ``Origin``, ``Triples``), from outside: what every
entry point that takes a handle answers in every state a caller can bring one into, and that ``ecb_reset`` forgets all of a run.
A run that was refused -- a push or a merge that failed after it had begun to change the table -- is a state too (``Run::refused``)."""
import ctypes as C

import numpy as np
import pytest

from alntools_amd import ecb

import refusal_streams as rs

pytestmark = pytest.mark.gpu

L, H, CELLS = 30, 4, 8
BIG = 1 << 14          # elements of every output buffer: far more than the few dozen reads here can fill


def _stream(seed, n_reads, first=0):
    """A few dozen reads of 1 .. 4 valid records each, read ids first .. first + n_reads - 1."""
    r = np.random.RandomState(seed)
    k = r.randint(1, 5, n_reads)
    rid = np.repeat(np.arange(first, first + n_reads), k).astype(np.uint32)
    n = len(rid)
    return dict(read_id=rid, locus=r.randint(0, L, n).astype(np.uint32), hapflag=(r.randint(0, H, n) << 16).astype(np.uint32),
                pos=r.randint(0, 100000, n).astype(np.int32), n_reads=n_reads, meta=(r.randint(0, CELLS, n_reads) | (r.randint(0, 2, n_reads) << 22)).astype(np.uint32))


NA, NB = 40, 64
A, A_NEXT, B = _stream(1, NA), _stream(2, 10, first=NA), _stream(3, NB)      # the first stream, one that continues it, a second, longer one
BAD = dict(A, read_id=A["read_id"] * 2)                                        # the run counter steps by two


def _long_keys(seed, n_reads):
    """Reads of one record on every locus: keys of L pairs, L - INL of them in the arena, told apart by their haplotypes."""
    r = np.random.RandomState(seed)
    n = n_reads * L
    return dict(read_id=np.repeat(np.arange(n_reads), L).astype(np.uint32), locus=np.tile(np.arange(L), n_reads).astype(np.uint32),
                hapflag=(r.randint(0, H, n) << 16).astype(np.uint32), pos=r.randint(0, 100000, n).astype(np.int32), n_reads=n_reads,
                meta=r.randint(0, CELLS, n_reads).astype(np.uint32))


TIGHT = rs.ARENA                                                               # pairs of the arena that LONG overruns
LONG = _long_keys(4, 700)
assert rs.key_pairs_beyond_the_slot(LONG) >= 4 * TIGHT                         # (the margin of test_gpu_refused_runs.py: no boundary is guessed)


class _Fix(object):
    """What the calls take besides the handle, made once: the streams on the device, a donor's exported table and finalized piece, buffers."""

    def __init__(self):
        import torch
        self.torch, self.dev = torch, torch.device("cuda:0")
        self.lib = ecb.load()
        up = lambda a: torch.from_numpy(a.view(np.int32)).to(self.dev)
        self.dA, self.dNext, self.dB, self.dBad, self.dLong = ({k: up(t[k]) for k in ("read_id", "locus", "hapflag", "pos", "meta")} for t in (A, A_NEXT, B, BAD, LONG))
        self.tiles = {id(d): ecb.tile_tuples(d["read_id"], d["locus"], d["hapflag"]) for d in (self.dA, self.dNext)}
        with self.new("plain") as d:                     # the donor: its table as exchanged between GPUs, and its finalized result as one piece
            d.push_device(self.dA["read_id"], self.dA["locus"], self.dA["hapflag"])
            self.ne, self.np_, _ = d.table_sizes()
            self.ent = torch.zeros(4 * BIG, dtype=torch.int64, device=self.dev)
            self.prs = torch.zeros(8 * BIG, dtype=torch.int64, device=self.dev)
            eo, po = d.table_export_parts_device(self.ent, self.prs, 0, 1)
            self.np_ = po[-1]
            self.ent2 = self.ent.clone()                 # (rebased in place)
            self.ctr = d.counters()
            s = d.finalize()
            self.piece = tuple(torch.zeros(BIG, dtype=torch.int32, device=self.dev) for _ in range(5)) + (s["n_ecs"], s["nnz_a"])
            d.export_piece_device(*self.piece[:5])
        with self.new("plain", arena=1 << 18, slots=4096) as d:         # a second donor: the table of LONG (fifteen times its pairs of arena)
            d.push_device(self.dLong["read_id"], self.dLong["locus"], self.dLong["hapflag"])
            self.long_ne, bound, _ = d.table_sizes()
            self.long_ent = torch.zeros(4 * self.long_ne, dtype=torch.int64, device=self.dev)
            self.long_prs = torch.zeros(bound, dtype=torch.int64, device=self.dev)
            self.long_np = d.table_export_parts_device(self.long_ent, self.long_prs, 0, 1)[1][-1]
        self.dbuf = [torch.zeros(8 * BIG, dtype=torch.int64, device=self.dev) for _ in range(7)]      # device outputs
        self.hbuf = [np.zeros(BIG, np.int64) for _ in range(8)]                                          # host outputs
        self.key1 = torch.zeros(2, dtype=torch.int64, device=self.dev)                                   # one merged EC: row {locus 0: mask 1}
        self.csr1 = (torch.tensor([0, 1], dtype=torch.int32, device=self.dev), torch.zeros(1, dtype=torch.int32, device=self.dev),
                     torch.ones(1, dtype=torch.int32, device=self.dev))
        self.tri = (torch.zeros(2, dtype=torch.int64, device=self.dev), torch.ones(2, dtype=torch.int32, device=self.dev),     # two triples of EC 0, cell 0, file 0
                    torch.zeros(2, dtype=torch.int32, device=self.dev), 2)
        torch.cuda.synchronize()

    def new(self, kind, arena=1 << 16, slots=1024):
        return ecb.EcBuilder(L, H, ec_capacity=slots, arena_capacity=arena, track_ranges=kind == "ranges", multisample=kind == "ms")


# ---- states -----------------------------------------------------------------------------------------------------------------------------------
def _push(F, b, d, kind):
    b.push_device(d["read_id"], d["locus"], d["hapflag"], d["pos"] if kind == "ranges" else None)
    if kind == "ms":
        b.push_cells_device(d["meta"], 0)


def _fresh(F, b, kind):
    pass


def _pushed(F, b, kind):
    _push(F, b, F.dA, kind)
    b.next = F.dNext


def _open_read(F, b, kind):
    b.push(A["read_id"], A["locus"], A["hapflag"], A["pos"] if kind == "ranges" else None)      # (the last read stays open: the next push may continue it)
    if kind == "ms":
        b.push_cells(A["meta"], 0)
    b.next = F.dNext


def _counted(F, b, kind):
    _pushed(F, b, kind)
    b.table_sizes()
    b.table_export_device(F.dbuf[0], F.dbuf[1], 0)


def _merged(F, b, kind):
    b.table_merge_device(F.ent, F.ne, F.prs, F.np_)
    b.add_counters(*F.ctr)


def _adopted(F, b, kind):
    b.table_adopt_device(F.ent, F.ne, F.prs, F.np_)
    b.add_counters(*F.ctr)


def _finalized(F, b, kind):
    _pushed(F, b, kind)
    b.finalize()


def _adopted_final(F, b, kind):
    _adopted(F, b, kind)
    b.finalize()


def _adopted_final_triples(F, b, kind):
    _adopted_final(F, b, kind)
    b.ms_adopt_triples_device([F.tri])


def _assembled(F, b, kind):
    b.assemble_ranges_device([F.piece], F.ctr[2], F.ctr[0], F.ctr[1])


def _filtered(F, b, kind):
    _finalized(F, b, kind)
    b.ms_filter_sizes(CELLS, 1)


def _refused(code, what):
    with pytest.raises(ecb.EcbError) as e:
        what()
    assert e.value.code == code, str(e.value)


def _push_refused_contract(F, b, kind):
    _refused(-5, lambda: _push(F, b, F.dBad, kind))


def _push_refused_arena(F, b, kind):
    _refused(-4, lambda: _push(F, b, F.dLong, kind))


def _merge_refused_arena(F, b, kind):
    _refused(-4, lambda: b.table_merge_device(F.long_ent, F.long_ne, F.long_prs, F.long_np))


#: state -> (how a fresh handle gets there, the kinds of handle it is reached with: the first is the one the refusals are recorded for)
STATES = {
    "fresh": (_fresh, ("plain", "ms", "ranges")), "pushed": (_pushed, ("plain", "ms", "ranges")), "open read": (_open_read, ("plain", "ranges")),
    "counted": (_counted, ("plain",)), "merged into": (_merged, ("plain",)), "adopted": (_adopted, ("plain",)),
    "finalized": (_finalized, ("plain", "ranges")), "ms finalized": (_finalized, ("ms",)), "ms adopted, finalized, no triples": (_adopted_final, ("ms",)),
    "ms adopted, finalized, triples": (_adopted_final_triples, ("ms",)), "assembled": (_assembled, ("plain", "ms")), "ms filtered": (_filtered, ("ms",)),
}


#: the states a refusal leaves: state -> (how a fresh handle gets there, kinds, (key arena, table slots) of the handle, code and text of the
#: refusal, what ecb_profile_kernel says).  They join STATES below RECORDED, where their rows are written down.
CONTRACT_TEXT = "read_id run counter violates the tuple contract (see ecb.h)"
ARENA_TEXT = "EC key arena exhausted (%d pairs): raise arena_capacity" % TIGHT
REFUSED = {
    "push refused, contract": (_push_refused_contract, ("plain", "ms", "ranges"), (), -5, CONTRACT_TEXT, "ks_std::k_stream<false, false>"),
    "push refused, arena": (_push_refused_arena, ("plain", "ms", "ranges"), (TIGHT, 4096), -4, ARENA_TEXT, "ks_std::k_stream<false, false>"),
    "merge refused, arena": (_merge_refused_arena, ("plain",), (TIGHT, 4096), -4, ARENA_TEXT, ""),
}
SHAPE = {s_: v_[2] for s_, v_ in REFUSED.items()}


def _enter(F, state, after_reset, kind=None):
    make, kinds = STATES[state]
    kind = kind or kinds[0]
    b = F.new(kind, *SHAPE.get(state, ()))
    b.kind, b.next = kind, F.dA                            # next: the stream a push continues the handle's with
    make(F, b, kind)
    if after_reset:
        b.reset()
        b.next = F.dA
    return b


# ---- every entry point of ecb.h that takes a handle, with arguments that are valid where the state allows the call ------------------------------
def _calls(F):
    lib, vp, u64 = F.lib, C.c_void_p, C.c_uint64
    P = lambda t: vp(t.data_ptr())
    H_ = lambda a: a.ctypes.data_as(vp)
    db, hb = [P(t) for t in F.dbuf], [H_(a) for a in F.hbuf]
    w = [u64() for _ in range(3)]
    wp = [C.byref(x) for x in w]
    host = {id(F.dA): A, id(F.dNext): A_NEXT}

    def push(b):
        t = host[id(b.next)]
        return lib.ecb_push(b._h, H_(t["read_id"]), H_(t["locus"]), H_(t["hapflag"]), H_(t["pos"]) if b.kind == "ranges" else None, len(t["read_id"]))

    def push_device(b):
        d = b.next
        return lib.ecb_push_device(b._h, P(d["read_id"]), P(d["locus"]), P(d["hapflag"]), P(d["pos"]) if b.kind == "ranges" else None, d["read_id"].numel())

    def merge_root(b):
        with F.new("plain") as shard:
            shard.push_device(F.dA["read_id"], F.dA["locus"], F.dA["hapflag"])
            return lib.ecb_merge((vp * 1)(shard._h.value), 1, b._h, C.byref(ecb.Sizes()))

    def kernel_name(b):
        b.text = (lib.ecb_profile_kernel(b._h) or b"").decode()
        return 0

    def last_error(b):
        b.text = (lib.ecb_last_error(b._h) or b"").decode()
        return 0

    batch = [(vp * 1)(F.ent.data_ptr()), (u64 * 1)(F.ne), (vp * 1)(F.prs.data_ptr()), (u64 * 1)(F.np_)]
    piece = [(vp * 1)(t.data_ptr()) for t in F.piece[:5]] + [(u64 * 1)(F.piece[5]), (u64 * 1)(F.piece[6])]
    tri = [(vp * 1)(t.data_ptr()) for t in F.tri[:3]] + [(u64 * 1)(F.tri[3])]
    return {
        "ecb_reset": lambda b: lib.ecb_reset(b._h),
        "ecb_push": push,
        "ecb_push_device": push_device,
        "ecb_push_device_tiled": lambda b: lib.ecb_push_device_tiled(b._h, P(F.tiles[id(b.next)]), b.next["read_id"].numel()),
        "ecb_hint_reads": lambda b: lib.ecb_hint_reads(b._h, 1000),
        "ecb_push_cells": lambda b: lib.ecb_push_cells(b._h, H_(A["meta"]), 0, NA),
        "ecb_push_cells_device": lambda b: lib.ecb_push_cells_device(b._h, P(F.dA["meta"]), 0, NA),
        "ecb_verify_device": lambda b: lib.ecb_verify_device(b._h, P(F.dA["read_id"]), P(F.dA["locus"]), P(F.dA["hapflag"]), F.dA["read_id"].numel(), wp[0], wp[1]),
        "ecb_verify_device_tiled": lambda b: lib.ecb_verify_device_tiled(b._h, P(F.tiles[id(F.dA)]), F.dA["read_id"].numel(), wp[0], wp[1]),
        "ecb_finalize": lambda b: lib.ecb_finalize(b._h, C.byref(ecb.Sizes())),
        "ecb_export": lambda b: lib.ecb_export(b._h, hb[0], hb[1], hb[2], None, None, None),
        "ecb_export with N": lambda b: lib.ecb_export(b._h, *hb[:6]),
        "ecb_export_device": lambda b: lib.ecb_export_device(b._h, *db[:6]),
        "ecb_export_ranges": lambda b: lib.ecb_export_ranges(b._h, hb[0]),
        "ecb_export_range_minmax": lambda b: lib.ecb_export_range_minmax(b._h, hb[0], hb[1]),
        "ecb_export_pairs": lambda b: lib.ecb_export_pairs(b._h, *hb[:4]),
        "ecb_ms_filter": lambda b: lib.ecb_ms_filter(b._h, CELLS, 1, C.byref(ecb.MsSizes())),
        "ecb_ms_export": lambda b: lib.ecb_ms_export(b._h, *hb[:7]),
        "ecb_export_read_ec": lambda b: lib.ecb_export_read_ec(b._h, hb[0]),
        "ecb_table_sizes": lambda b: lib.ecb_table_sizes(b._h, *wp),
        "ecb_table_export_device": lambda b: lib.ecb_table_export_device(b._h, db[0], db[1], 0),
        "ecb_table_export_parts_device": lambda b: lib.ecb_table_export_parts_device(b._h, db[0], db[1], 0, 4, (u64 * 5)(), (u64 * 5)()),
        "ecb_table_merge_device": lambda b: lib.ecb_table_merge_device(b._h, P(F.ent), F.ne, P(F.prs), F.np_),
        "ecb_table_merge_batch_device": lambda b: lib.ecb_table_merge_batch_device(b._h, 1, *batch),
        "ecb_table_adopt_device": lambda b: lib.ecb_table_adopt_device(b._h, P(F.ent), F.ne, P(F.prs), F.np_),
        "ecb_table_adopt_batch_device": lambda b: lib.ecb_table_adopt_batch_device(b._h, 1, *batch),
        "ecb_table_rebase_device": lambda b: lib.ecb_table_rebase_device(b._h, P(F.ent2), F.ne, 5),
        "ecb_export_firsts_device": lambda b: lib.ecb_export_firsts_device(b._h, db[0]),
        "ecb_assemble_ranges_device": lambda b: lib.ecb_assemble_ranges_device(b._h, 1, *piece, F.ctr[2], F.ctr[0], F.ctr[1], C.byref(ecb.Sizes())),
        "ecb_export_ec_keys_device": lambda b: lib.ecb_export_ec_keys_device(b._h, db[0]),
        "ecb_ms_local_triples_device": lambda b: lib.ecb_ms_local_triples_device(b._h, P(F.key1), P(F.csr1[0]), P(F.csr1[1]), P(F.csr1[2]), 1, 0, db[2], db[3], db[4], wp[0]),
        "ecb_ms_adopt_triples_device": lambda b: lib.ecb_ms_adopt_triples_device(b._h, 1, *tri, wp[0]),
        "ecb_counters": lambda b: lib.ecb_counters(b._h, *wp),
        "ecb_add_counters": lambda b: lib.ecb_add_counters(b._h, 1, 1, 1),
        "ecb_profile": lambda b: lib.ecb_profile(b._h, 1),
        "ecb_profile_read": lambda b: lib.ecb_profile_read(b._h, C.byref(C.c_double()), wp[0], wp[1]),
        "ecb_profile_kernel": kernel_name,
        "ecb_last_error": last_error,
        "ecb_merge as the root": merge_root,
    }


def _observe(F, calls, state, after_reset, call):
    """-> (return code, ecb_last_error(h)) of `call` on a new handle brought into `state` (ecb_destroy ends every one of them)."""
    b = _enter(F, state, after_reset)
    try:
        b.text = None
        rc = calls[call](b)
        F.torch.cuda.synchronize()
        return rc, (F.lib.ecb_last_error(b._h) or b"").decode() if b.text is None else b.text
    finally:
        b.close()


_S = lambda state, after_reset: state + (", reset" if after_reset else "")

# Recorded by running this same table (`python tests/test_gpu_handle_states.py`) against a library built from the commit before the handle was
# given one per-run record (9c0c637), not from the code under test: call -> {(return code, ecb_last_error(h)): the states that answer so}.
# (For ecb_profile_kernel and ecb_last_error, which return a text, the text stands in the second place.  ALL: every state.)
ALL = [_S(s_, r_) for s_ in STATES for r_ in (False, True)]
RECORDED = {
    'ecb_reset': {
        (0, ''): ALL,
    },
    'ecb_push': {
        (0, ''): [
            'fresh', 'fresh, reset', 'pushed', 'pushed, reset', 'open read', 'open read, reset', 'counted, reset', 'merged into, reset',
            'adopted, reset', 'finalized, reset', 'ms finalized, reset', 'ms adopted, finalized, no triples, reset',
            'ms adopted, finalized, triples, reset', 'assembled, reset', 'ms filtered, reset'],
        (-6, 'push after finalize / table export'): [
            'counted', 'merged into', 'adopted', 'finalized', 'ms finalized', 'ms adopted, finalized, no triples', 'ms adopted, finalized, triples',
            'assembled', 'ms filtered'],
    },
    'ecb_push_device': {
        (0, ''): [
            'fresh', 'fresh, reset', 'pushed', 'pushed, reset', 'open read, reset', 'counted, reset', 'merged into, reset', 'adopted, reset',
            'finalized, reset', 'ms finalized, reset', 'ms adopted, finalized, no triples, reset', 'ms adopted, finalized, triples, reset',
            'assembled, reset', 'ms filtered, reset'],
        (-6, 'ecb_push_device while a host push has an open read'): [
            'open read'],
        (-6, 'push after finalize / table export'): [
            'counted', 'merged into', 'adopted', 'finalized', 'ms finalized', 'ms adopted, finalized, no triples', 'ms adopted, finalized, triples',
            'assembled', 'ms filtered'],
    },
    'ecb_push_device_tiled': {
        (0, ''): [
            'fresh', 'fresh, reset', 'pushed', 'pushed, reset', 'open read, reset', 'counted, reset', 'merged into, reset', 'adopted, reset',
            'finalized, reset', 'ms finalized, reset', 'ms adopted, finalized, no triples, reset', 'ms adopted, finalized, triples, reset',
            'assembled, reset', 'ms filtered, reset'],
        (-6, 'ecb_push_device_tiled while a host push has an open read'): [
            'open read'],
        (-6, 'push after finalize / table export'): [
            'counted', 'merged into', 'adopted', 'finalized', 'ms finalized', 'ms adopted, finalized, no triples', 'ms adopted, finalized, triples',
            'assembled', 'ms filtered'],
    },
    'ecb_hint_reads': {
        (0, ''): ALL,
    },
    'ecb_push_cells': {
        (-6, 'handle was created without ECB_F_MULTISAMPLE'): [
            'fresh', 'fresh, reset', 'pushed', 'pushed, reset', 'open read', 'open read, reset', 'counted', 'counted, reset', 'merged into',
            'merged into, reset', 'adopted', 'adopted, reset', 'finalized', 'finalized, reset', 'assembled', 'assembled, reset'],
        (-6, 'push after finalize'): [
            'ms finalized', 'ms adopted, finalized, no triples', 'ms adopted, finalized, triples', 'ms filtered'],
        (0, ''): [
            'ms finalized, reset', 'ms adopted, finalized, no triples, reset', 'ms adopted, finalized, triples, reset', 'ms filtered, reset'],
    },
    'ecb_push_cells_device': {
        (-6, 'handle was created without ECB_F_MULTISAMPLE'): [
            'fresh', 'fresh, reset', 'pushed', 'pushed, reset', 'open read', 'open read, reset', 'counted', 'counted, reset', 'merged into',
            'merged into, reset', 'adopted', 'adopted, reset', 'finalized', 'finalized, reset', 'assembled', 'assembled, reset'],
        (-6, 'push after finalize'): [
            'ms finalized', 'ms adopted, finalized, no triples', 'ms adopted, finalized, triples', 'ms filtered'],
        (0, ''): [
            'ms finalized, reset', 'ms adopted, finalized, no triples, reset', 'ms adopted, finalized, triples, reset', 'ms filtered, reset'],
    },
    'ecb_verify_device': {
        (-5, 'read_id run counter violates the tuple contract (see ecb.h)'): [
            'fresh', 'fresh, reset', 'pushed, reset', 'open read', 'open read, reset', 'counted, reset', 'merged into', 'merged into, reset',
            'adopted', 'adopted, reset', 'finalized, reset', 'ms finalized, reset', 'ms adopted, finalized, no triples',
            'ms adopted, finalized, no triples, reset', 'ms adopted, finalized, triples', 'ms adopted, finalized, triples, reset', 'assembled',
            'assembled, reset', 'ms filtered, reset'],
        (0, ''): [
            'pushed', 'counted', 'finalized', 'ms finalized', 'ms filtered'],
    },
    'ecb_verify_device_tiled': {
        (-5, 'read_id run counter violates the tuple contract (see ecb.h)'): [
            'fresh', 'fresh, reset', 'pushed, reset', 'open read', 'open read, reset', 'counted, reset', 'merged into', 'merged into, reset',
            'adopted', 'adopted, reset', 'finalized, reset', 'ms finalized, reset', 'ms adopted, finalized, no triples',
            'ms adopted, finalized, no triples, reset', 'ms adopted, finalized, triples', 'ms adopted, finalized, triples, reset', 'assembled',
            'assembled, reset', 'ms filtered, reset'],
        (0, ''): [
            'pushed', 'counted', 'finalized', 'ms finalized', 'ms filtered'],
    },
    'ecb_finalize': {
        (-7, 'no valid alignments: nothing to build (the reference fails here too)'): [
            'fresh', 'fresh, reset', 'pushed, reset', 'open read, reset', 'counted, reset', 'merged into, reset', 'adopted, reset',
            'finalized, reset', 'ms finalized, reset', 'ms adopted, finalized, no triples, reset', 'ms adopted, finalized, triples, reset',
            'assembled, reset', 'ms filtered, reset'],
        (0, ''): [
            'pushed', 'open read', 'counted', 'merged into', 'adopted', 'finalized', 'ms finalized', 'ms adopted, finalized, no triples',
            'ms adopted, finalized, triples', 'assembled', 'ms filtered'],
    },
    'ecb_export': {
        (-6, 'export before finalize'): [
            'fresh', 'fresh, reset', 'pushed', 'pushed, reset', 'open read', 'open read, reset', 'counted', 'counted, reset', 'merged into',
            'merged into, reset', 'adopted', 'adopted, reset', 'finalized, reset', 'ms finalized, reset', 'ms adopted, finalized, no triples, reset',
            'ms adopted, finalized, triples, reset', 'assembled, reset', 'ms filtered, reset'],
        (0, ''): [
            'finalized', 'ms finalized', 'ms adopted, finalized, no triples', 'ms adopted, finalized, triples', 'assembled', 'ms filtered'],
    },
    'ecb_export with N': {
        (-6, 'export before finalize'): [
            'fresh', 'fresh, reset', 'pushed', 'pushed, reset', 'open read', 'open read, reset', 'counted', 'counted, reset', 'merged into',
            'merged into, reset', 'adopted', 'adopted, reset', 'finalized, reset', 'ms finalized, reset', 'ms adopted, finalized, no triples, reset',
            'ms adopted, finalized, triples, reset', 'assembled, reset', 'ms filtered, reset'],
        (0, ''): [
            'finalized', 'assembled'],
        (-6, 'multisample: N comes from ecb_export_pairs'): [
            'ms finalized', 'ms adopted, finalized, no triples', 'ms adopted, finalized, triples', 'ms filtered'],
    },
    'ecb_export_device': {
        (-6, 'export before finalize'): [
            'fresh', 'fresh, reset', 'pushed', 'pushed, reset', 'open read', 'open read, reset', 'counted', 'counted, reset', 'merged into',
            'merged into, reset', 'adopted', 'adopted, reset', 'finalized, reset', 'ms finalized, reset', 'ms adopted, finalized, no triples, reset',
            'ms adopted, finalized, triples, reset', 'assembled, reset', 'ms filtered, reset'],
        (0, ''): [
            'finalized', 'ms finalized', 'ms adopted, finalized, no triples', 'ms adopted, finalized, triples', 'assembled', 'ms filtered'],
    },
    'ecb_export_ranges': {
        (-6, 'handle was created without ECB_F_RANGES'): ALL,
    },
    'ecb_export_range_minmax': {
        (-6, 'handle was created without ECB_F_RANGES'): ALL,
    },
    'ecb_export_pairs': {
        (-6, 'no multisample result'): [
            'fresh', 'fresh, reset', 'pushed', 'pushed, reset', 'open read', 'open read, reset', 'counted', 'counted, reset', 'merged into',
            'merged into, reset', 'adopted', 'adopted, reset', 'finalized', 'finalized, reset', 'ms finalized, reset',
            'ms adopted, finalized, no triples, reset', 'ms adopted, finalized, triples, reset', 'assembled', 'assembled, reset',
            'ms filtered, reset'],
        (0, ''): [
            'ms finalized', 'ms adopted, finalized, triples', 'ms filtered'],
        (-6, 'multisample across GPUs: no triples adopted yet (ecb_ms_adopt_triples_device)'): [
            'ms adopted, finalized, no triples'],
    },
    'ecb_ms_filter': {
        (-6, 'no multisample result'): [
            'fresh', 'fresh, reset', 'pushed', 'pushed, reset', 'open read', 'open read, reset', 'counted', 'counted, reset', 'merged into',
            'merged into, reset', 'adopted', 'adopted, reset', 'finalized', 'finalized, reset', 'ms finalized, reset',
            'ms adopted, finalized, no triples, reset', 'ms adopted, finalized, triples, reset', 'assembled', 'assembled, reset',
            'ms filtered, reset'],
        (0, ''): [
            'ms finalized', 'ms adopted, finalized, triples', 'ms filtered'],
        (-6, 'multisample across GPUs: no triples adopted yet (ecb_ms_adopt_triples_device)'): [
            'ms adopted, finalized, no triples'],
    },
    'ecb_ms_export': {
        (-6, 'ecb_ms_export before ecb_ms_filter'): [
            'fresh', 'fresh, reset', 'pushed', 'pushed, reset', 'open read', 'open read, reset', 'counted', 'counted, reset', 'merged into',
            'merged into, reset', 'adopted', 'adopted, reset', 'finalized', 'finalized, reset', 'ms finalized', 'ms finalized, reset',
            'ms adopted, finalized, no triples', 'ms adopted, finalized, no triples, reset', 'ms adopted, finalized, triples',
            'ms adopted, finalized, triples, reset', 'assembled', 'assembled, reset', 'ms filtered, reset'],
        (0, ''): [
            'ms filtered'],
    },
    'ecb_export_read_ec': {
        (-6, 'export before finalize'): [
            'fresh', 'fresh, reset', 'pushed', 'pushed, reset', 'open read', 'open read, reset', 'counted', 'counted, reset', 'merged into',
            'merged into, reset', 'adopted', 'adopted, reset', 'finalized, reset', 'ms finalized, reset', 'ms adopted, finalized, no triples, reset',
            'ms adopted, finalized, triples, reset', 'assembled, reset', 'ms filtered, reset'],
        (0, ''): [
            'finalized', 'ms finalized', 'ms filtered'],
        (-6, 'per-read EC ids are not kept across a multi-GPU merge'): [
            'ms adopted, finalized, no triples', 'ms adopted, finalized, triples', 'assembled'],
    },
    'ecb_table_sizes': {
        (0, ''): ALL,
    },
    'ecb_table_export_device': {
        (0, ''): ALL,
    },
    'ecb_table_export_parts_device': {
        (0, ''): ALL,
    },
    'ecb_table_merge_device': {
        (0, ''): [
            'fresh', 'fresh, reset', 'pushed', 'pushed, reset', 'open read', 'open read, reset', 'counted', 'counted, reset', 'merged into',
            'merged into, reset', 'adopted, reset', 'finalized, reset', 'ms finalized, reset', 'ms adopted, finalized, no triples, reset',
            'ms adopted, finalized, triples, reset', 'assembled, reset', 'ms filtered, reset'],
        (-6, 'merge into a table that adopted entries'): [
            'adopted'],
        (-6, 'merge after finalize'): [
            'finalized', 'ms finalized', 'ms adopted, finalized, no triples', 'ms adopted, finalized, triples', 'assembled', 'ms filtered'],
    },
    'ecb_table_merge_batch_device': {
        (0, ''): [
            'fresh', 'fresh, reset', 'pushed', 'pushed, reset', 'open read', 'open read, reset', 'counted', 'counted, reset', 'merged into',
            'merged into, reset', 'adopted, reset', 'finalized, reset', 'ms finalized, reset', 'ms adopted, finalized, no triples, reset',
            'ms adopted, finalized, triples, reset', 'assembled, reset', 'ms filtered, reset'],
        (-6, 'merge into a table that adopted entries'): [
            'adopted'],
        (-6, 'merge after finalize'): [
            'finalized', 'ms finalized', 'ms adopted, finalized, no triples', 'ms adopted, finalized, triples', 'assembled', 'ms filtered'],
    },
    'ecb_table_adopt_device': {
        (0, ''): [
            'fresh', 'fresh, reset', 'pushed, reset', 'open read, reset', 'counted, reset', 'merged into, reset', 'adopted', 'adopted, reset',
            'finalized, reset', 'ms finalized, reset', 'ms adopted, finalized, no triples, reset', 'ms adopted, finalized, triples, reset',
            'assembled, reset', 'ms filtered, reset'],
        (-6, 'adopt needs an empty handle (use ecb_table_merge_device to add to a built table)'): [
            'pushed', 'open read', 'counted', 'merged into'],
        (-6, 'adopt after finalize'): [
            'finalized', 'ms finalized', 'ms adopted, finalized, no triples', 'ms adopted, finalized, triples', 'assembled', 'ms filtered'],
    },
    'ecb_table_adopt_batch_device': {
        (0, ''): [
            'fresh', 'fresh, reset', 'pushed, reset', 'open read, reset', 'counted, reset', 'merged into, reset', 'adopted', 'adopted, reset',
            'finalized, reset', 'ms finalized, reset', 'ms adopted, finalized, no triples, reset', 'ms adopted, finalized, triples, reset',
            'assembled, reset', 'ms filtered, reset'],
        (-6, 'adopt needs an empty handle (use ecb_table_merge_device to add to a built table)'): [
            'pushed', 'open read', 'counted', 'merged into'],
        (-6, 'adopt after finalize'): [
            'finalized', 'ms finalized', 'ms adopted, finalized, no triples', 'ms adopted, finalized, triples', 'assembled', 'ms filtered'],
    },
    'ecb_table_rebase_device': {
        (0, ''): ALL,
    },
    'ecb_export_firsts_device': {
        (-6, 'first reads are exported from a finalized table'): [
            'fresh', 'fresh, reset', 'pushed', 'pushed, reset', 'open read', 'open read, reset', 'counted', 'counted, reset', 'merged into',
            'merged into, reset', 'adopted', 'adopted, reset', 'finalized, reset', 'ms finalized, reset', 'ms adopted, finalized, no triples, reset',
            'ms adopted, finalized, triples, reset', 'assembled', 'assembled, reset', 'ms filtered, reset'],
        (0, ''): [
            'finalized', 'ms finalized', 'ms adopted, finalized, no triples', 'ms adopted, finalized, triples', 'ms filtered'],
    },
    'ecb_assemble_ranges_device': {
        (0, ''): [
            'fresh', 'fresh, reset', 'pushed, reset', 'open read, reset', 'counted, reset', 'merged into, reset', 'adopted, reset',
            'finalized, reset', 'ms finalized, reset', 'ms adopted, finalized, no triples, reset', 'ms adopted, finalized, triples, reset',
            'assembled, reset', 'ms filtered, reset'],
        (-6, 'assembling needs an empty handle'): [
            'pushed', 'open read', 'counted', 'merged into', 'adopted', 'finalized', 'ms finalized', 'ms adopted, finalized, no triples',
            'ms adopted, finalized, triples', 'assembled', 'ms filtered'],
    },
    'ecb_export_ec_keys_device': {
        (-6, 'export before finalize'): [
            'fresh', 'fresh, reset', 'pushed', 'pushed, reset', 'open read', 'open read, reset', 'counted', 'counted, reset', 'merged into',
            'merged into, reset', 'adopted', 'adopted, reset', 'finalized, reset', 'ms finalized, reset', 'ms adopted, finalized, no triples, reset',
            'ms adopted, finalized, triples, reset', 'assembled, reset', 'ms filtered, reset'],
        (0, ''): [
            'finalized', 'ms finalized', 'ms adopted, finalized, no triples', 'ms adopted, finalized, triples', 'assembled', 'ms filtered'],
    },
    'ecb_ms_local_triples_device': {
        (-6, 'handle was created without ECB_F_MULTISAMPLE'): [
            'fresh', 'fresh, reset', 'pushed', 'pushed, reset', 'open read', 'open read, reset', 'counted', 'counted, reset', 'merged into',
            'merged into, reset', 'adopted', 'adopted, reset', 'finalized', 'finalized, reset', 'assembled', 'assembled, reset'],
        (-6, "a shard's triples come from the handle its reads were pushed into"): [
            'ms finalized', 'ms adopted, finalized, no triples', 'ms adopted, finalized, triples', 'ms filtered'],
        (0, ''): [
            'ms finalized, reset', 'ms adopted, finalized, no triples, reset', 'ms adopted, finalized, triples, reset', 'ms filtered, reset'],
    },
    'ecb_ms_adopt_triples_device': {
        (-6, 'handle was created without ECB_F_MULTISAMPLE'): [
            'fresh', 'fresh, reset', 'pushed', 'pushed, reset', 'open read', 'open read, reset', 'counted', 'counted, reset', 'merged into',
            'merged into, reset', 'adopted', 'adopted, reset', 'finalized', 'finalized, reset', 'assembled', 'assembled, reset'],
        (-6, 'triples are adopted by the finalized handle that adopted the merged ECs (or assembled their ranges)'): [
            'ms finalized', 'ms finalized, reset', 'ms adopted, finalized, no triples, reset', 'ms adopted, finalized, triples, reset',
            'ms filtered', 'ms filtered, reset'],
        (0, ''): [
            'ms adopted, finalized, no triples', 'ms adopted, finalized, triples'],
    },
    'ecb_counters': {
        (0, ''): ALL,
    },
    'ecb_add_counters': {
        (0, ''): ALL,
    },
    'ecb_profile': {
        (0, ''): ALL,
    },
    'ecb_profile_read': {
        (0, ''): ALL,
    },
    'ecb_profile_kernel': {
        (0, ''): [
            'fresh', 'fresh, reset', 'merged into', 'merged into, reset', 'adopted', 'adopted, reset', 'ms adopted, finalized, no triples',
            'ms adopted, finalized, no triples, reset', 'ms adopted, finalized, triples', 'ms adopted, finalized, triples, reset', 'assembled',
            'assembled, reset'],
        (0, 'ks_std::k_stream<false, false>'): [
            'pushed', 'pushed, reset', 'open read', 'open read, reset', 'counted', 'counted, reset', 'finalized', 'finalized, reset', 'ms finalized',
            'ms finalized, reset', 'ms filtered', 'ms filtered, reset'],
    },
    'ecb_last_error': {
        (0, ''): ALL,
    },
    'ecb_merge as the root': {
        (0, ''): [
            'fresh', 'fresh, reset', 'pushed, reset', 'open read, reset', 'counted, reset', 'merged into, reset', 'adopted, reset',
            'finalized, reset', 'assembled, reset'],
        (-6, 'assembling needs an empty handle'): [
            'pushed', 'open read', 'counted', 'merged into', 'adopted', 'finalized', 'assembled'],
        (-6, 'ecb_merge: single-sample handles (the multisample merge has a second exchange: alntools_amd/dist.py)'): [
            'ms finalized', 'ms finalized, reset', 'ms adopted, finalized, no triples', 'ms adopted, finalized, no triples, reset',
            'ms adopted, finalized, triples', 'ms adopted, finalized, triples, reset', 'ms filtered', 'ms filtered, reset'],
    },
}


# The states after a refusal are not recorded from a library -- the parent's ran ecb_finalize's kernels over a half-built table there -- but
# written down from the rule of include/ecb.h: a refused run answers every call but ecb_reset (ecb_destroy), ecb_last_error and ecb_profile*
# with ECB_ERR_STATE and a text that names the refusal, before anything else is looked at; the calls that succeed leave the refusal's text
# in place (ecb_reset forgets it).  After ecb_reset the handle answers as "fresh, reset" does -- as "pushed, reset" where a push was refused,
# which is the same in every row but ecb_profile_kernel's: the handle keeps naming the last kernel it launched.
RECORDED = {c_: {k_: list(v_) for k_, v_ in by_.items()} for c_, by_ in RECORDED.items()}       # (ALL was one list)
for s_, (make_, kinds_, _, code_, text_, kernel_) in REFUSED.items():
    STATES[s_] = (make_, kinds_)
    for c_, by_ in RECORDED.items():
        got_ = {"ecb_reset": (0, ""), "ecb_profile": (0, text_), "ecb_profile_read": (0, text_), "ecb_last_error": (0, text_),
                "ecb_profile_kernel": (0, kernel_)}.get(c_, (-6, "this run was refused (%d: %s): ecb_reset the handle" % (code_, text_)))
        by_.setdefault(got_, []).append(s_)
        twin_ = "pushed, reset" if kernel_ else "fresh, reset"
        next(v_ for v_ in by_.values() if twin_ in v_).append(s_ + ", reset")


def test_every_entry_point_answers_as_before_in_every_state():
    """Every (state, entry point) pair: a new handle is brought into the state -- fresh, pushed, a host push with an open read, counted by a
    table export, merged into, adopted, finalized, finalized multisample with its own triples / adopted without triples / adopted with
    triples, assembled, filtered, and each of these followed by ``ecb_reset`` -- the entry point is called once with arguments that are
    otherwise valid, and the return code and ``ecb_last_error(h)`` are compared with literals recorded from the parent commit's library.
    The states a refusal leaves -- a push that broke the tuple contract, a push and a merge that overran a key arena of 4 096 pairs -- and
    their resets are pinned to the rule of ``include/ecb.h`` (the rows are built below ``RECORDED``).
    A pair whose call succeeds is pinned to ECB_OK (0).  No pair is left out: the table is checked against ``ecb.SYMBOLS``."""
    F = _Fix()
    calls = _calls(F)
    stateless = ("csr", "hapcsc", "apply", "combine", "salmon", "release")
    assert {c.split(" ")[0] for c in calls} | {"ecb_create", "ecb_destroy", "ecb_abi_version", "ecb_device_count"} == \
        {s for s in ecb.SYMBOLS if s.split("_")[1] not in stateless}
    states = [_S(s, r) for s in STATES for r in (False, True)]
    assert set(RECORDED) == set(calls)
    wrong = []
    for call in calls:
        want = {s: got for got, ss in RECORDED[call].items() for s in ss}
        assert sorted(want) == sorted(states), call           # every state, once
        for state in STATES:
            for after_reset in (False, True):
                got = _observe(F, calls, state, after_reset, call)
                print(call, "|", _S(state, after_reset), "|", got)
                if got != want[_S(state, after_reset)]:
                    wrong.append((call, _S(state, after_reset), got, want[_S(state, after_reset)]))
    assert not wrong, wrong[:8]


def _results(F, b, t):
    """Everything a caller can read of a finalized handle that was given stream `t`."""
    out = dict(sizes=b.finalize(), counters=b.counters())
    out.update(b.export())
    if b.kind == "ms":
        out.update({"pairs_" + k: v for k, v in b.export_pairs().items()})
        out.update({"filter_" + k: v for k, v in b.ms_filter(CELLS, 2).items()})
    out["read_ec"] = b.export_read_ec()
    if b.kind == "ranges":
        out["ranges"] = b.export_ranges()
        out["range_min"], out["range_max"] = b.export_range_minmax()
    return out


@pytest.mark.parametrize("state", sorted(STATES))
def test_reset_forgets_everything_of_the_run_before(state):
    """From every state, with every kind of handle the state is reached with (plain, ECB_F_MULTISAMPLE, ECB_F_RANGES): ``ecb_reset``, then a
    second, different and LONGER stream (the shorter one: test_reads_bound_given_up_front_and_a_handle_reused_for_a_shorter_stream),
    finalized and exported -- every exported array, ``ecb_counters``, ``ecb_export_read_ec``, the ranges, the triples and a filter at one
    threshold are bit for bit those of a fresh handle that was given the second stream only (``ecb.hip: ecb_reset`` ends in ``run = Run{}``)."""
    F = _Fix()
    for kind in STATES[state][1]:
        with F.new(kind) as fresh:
            fresh.kind = kind
            _push(F, fresh, F.dB, kind)
            want = _results(F, fresh, B)
        b = _enter(F, state, True, kind)
        try:
            _push(F, b, F.dB, kind)
            got = _results(F, b, B)
        finally:
            b.close()
        assert sorted(got) == sorted(want)
        for k in want:
            assert np.array_equal(got[k], want[k]) if isinstance(want[k], np.ndarray) else got[k] == want[k], (kind, k)
        assert got["sizes"]["n_reads"] == NB


if __name__ == "__main__":                                   # print the table to record
    F_ = _Fix()
    calls_ = _calls(F_)
    table = {}
    for call_ in calls_:
        for state_ in STATES:
            for r_ in (False, True):
                table.setdefault(call_, {}).setdefault(_observe(F_, calls_, state_, r_, call_), []).append(_S(state_, r_))
    print("RECORDED = {")
    for call_, by in table.items():
        print("    %r: {" % call_)
        for got_, ss_ in by.items():
            print("        %r: %r," % (got_, ss_))
        print("    },")
    print("}")
