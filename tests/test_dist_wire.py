"""What the multi-rank protocol (alntools_amd/dist.py) puts on the wire, on CPU / gloo: every rank's ordered trace of
``torch.distributed`` calls -- each batch of ``batch_isend_irecv`` with its (isend | irecv, peer, dtype, numel) in order -- and of engine
calls (``tools/dist_wire_trace.py``) against ``golden/dist_wire_trace.json``, recorded from the commit before the gather-to-root and the
rank scaffold were written once (``python tools/dist_wire_trace.py --tree <that checkout> --out tests/golden/dist_wire_trace.json``).
RCCL pairs messages up by their order within a batch and cannot run two ranks on one GPU: this is where a change of order shows.
Then the rule of ``HostStagedEngine`` on a stub engine, and ``all_gather_bytes``."""
import json
import os
import pickle
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from alntools_amd import dist as ecdist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tools"))
import dist_wire_trace as wt      # noqa: E402

FROZEN = json.load(open(os.path.join(HERE, "golden", "dist_wire_trace.json")))


def test_the_frozen_trace_has_exactly_the_cases():
    assert sorted(FROZEN) == sorted(wt.case_name(*c) for c in wt.CASES)


@pytest.mark.parametrize("case", wt.CASES, ids=lambda c: wt.case_name(*c))
def test_every_rank_sends_and_asks_what_it_did(case):
    got = wt.run_case(os.path.join(HERE, ".."), *case)
    want = FROZEN[wt.case_name(*case)]
    assert len(got) == len(want)
    for rank, (g, w) in enumerate(zip(got, want)):
        for i, (ge, we) in enumerate(zip(g, w)):
            assert ge == we, "rank %d, event %d" % (rank, i)
        assert len(g) == len(w), "rank %d" % rank


# --- HostStagedEngine: one rule, two exceptions ------------------------------------------------------------------------------

INTERFACE = ("table_sizes", "counters", "table_export", "table_export_parts", "table_merge", "table_merge_many", "table_adopt",
             "table_adopt_many", "table_rebase", "add_counters", "finalize_range", "assemble_ranges", "ec_keys", "ms_local_triples",
             "ms_adopt_triples")       # (the module text of dist.py, and the second exchange's three)


class Marked(torch.Tensor):
    """A CPU tensor that notes where it is sent and stays where it is."""

    def to(self, device, *a, **k):
        self.sent.append(torch.device(device).type)
        return self

    def cpu(self):
        return self.to("cpu")


def marked():
    t = torch.zeros(3, dtype=torch.int64).as_subclass(Marked)
    t.sent = []
    return t


def _sent(a):
    if isinstance(a, Marked):
        return a.sent
    return type(a)(_sent(x) for x in a) if isinstance(a, (list, tuple)) else a


class StubEngine(object):
    """Notes every call and returns what it is told to.  It calls its device ``meta``, so that up and down are two places."""
    device = torch.device("meta")
    b = "the builder"

    def __init__(self):
        self.calls, self.result = [], None

    def __getattr__(self, name):
        if name not in INTERFACE:
            raise AttributeError(name)

        def call(*a):
            self.calls.append((name, a))
            return self.result
        return call


def test_staged_engine_keeps_its_attributes():
    inner = StubEngine()
    eng = ecdist.HostStagedEngine(inner)
    assert eng.e is inner and eng.b == "the builder" and eng.dev == torch.device("meta")
    assert eng.device == ecdist.HostStagedEngine.device == torch.device("cpu")
    assert all(callable(getattr(eng, name)) for name in INTERFACE)


@pytest.mark.parametrize("name", [n for n in INTERFACE if n not in ("table_rebase", "table_export_parts")])
def test_staged_engine_moves_nested_tensors_up_and_results_down(name):
    inner = StubEngine()
    eng = ecdist.HostStagedEngine(inner)
    args = (marked(), 4, [(marked(), 1, marked(), 2), (marked(), 3)])
    inner.result = (marked(), 5, [(marked(), 7)])
    out = getattr(eng, name)(*args)
    (called, seen), = inner.calls
    assert called == name
    assert _sent(seen) == (["meta"], 4, [(["meta"], 1, ["meta"], 2), (["meta"], 3)])      # every tensor went up, once, and reached the engine
    assert seen[0] is args[0] and seen[2][1][0] is args[2][1][0]
    assert _sent(out) == (["cpu"], 5, [(["cpu"], 7)]) and out[0] is inner.result[0]         # every tensor of the result came down
    inner.result = None
    assert getattr(eng, name)() is None


def test_staged_rebase_with_nothing_to_do_returns_its_argument():
    inner = StubEngine()
    eng = ecdist.HostStagedEngine(inner)
    ent = marked()
    assert eng.table_rebase(ent, 2, 0) is ent and eng.table_rebase(ent, 0, 9) is ent
    assert not inner.calls and not ent.sent
    inner.result = marked()
    assert eng.table_rebase(ent, 2, 9) is inner.result
    assert inner.calls == [("table_rebase", (ent, 2, 9))] and ent.sent == ["meta"]
    assert inner.result.sent == []                                      # (stays up for the merge that follows)


def test_staged_export_parts_hands_the_offset_lists_on():
    inner = StubEngine()
    eng = ecdist.HostStagedEngine(inner)
    eoff, poff = [0, 1, 2], [0, 3, 3]
    inner.result = (marked(), marked(), eoff, poff)
    ent, prs, eo, po = eng.table_export_parts(0, 2)
    assert inner.calls == [("table_export_parts", (0, 2))]
    assert ent.sent == prs.sent == ["cpu"] and eo is eoff and po is poff


# --- all_gather_bytes ---------------------------------------------------------------------------------------------------------

def _bytes_rank(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    log = []
    undo = wt.record_dist(dist, log)
    try:
        got = ecdist.all_gather_bytes(_blob(rank), torch.device("cpu"))
    finally:
        undo()
    with open(os.path.join(out_dir, "rank%d.pkl" % rank), "wb") as fh:
        pickle.dump((got, log), fh)
    dist.barrier()
    dist.destroy_process_group()


def _blob(rank):
    return (b"", pickle.dumps(["cell %d" % i for i in range(40)]), b"\x00\xff")[rank]


def test_all_gather_bytes_is_two_all_gathers_padded_to_the_longest(tmp_path):
    """Every rank gets every rank's bytes, an empty one too; on the wire: the lengths, then the blobs padded to the longest."""
    world = 3
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    mp.spawn(_bytes_rank, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    longest = max(len(_blob(r)) for r in range(world))
    for rank in range(world):
        got, log = pickle.load(open(str(tmp_path / ("rank%d.pkl" % rank)), "rb"))
        assert got == [_blob(r) for r in range(world)]
        assert log == [["dist", "all_gather_into_tensor", "torch.int64", 1, {}], ["dist", "all_gather_into_tensor", "torch.uint8", longest, {}]]
