#!/usr/bin/env python
"""What the multi-rank protocol of ``alntools_amd/dist.py`` puts on the wire and asks of its engines, recorded on the CPU over gloo
with the ``OracleEngine`` of ``tests/test_dist_gloo.py``.

    python tools/dist_wire_trace.py [--tree DIR] [--out FILE]     one sha256 per case and one over all cases

``--tree``: the checkout whose ``alntools_amd`` is driven (default: this one), so that two commits can be compared by the same driver.
Inside every rank, in order: every ``torch.distributed`` call of the protocol -- the collectives with dtype, numel and src / op, every
batch handed to ``batch_isend_irecv`` as its ordered list of (isend | irecv, peer, dtype, numel) -- and every engine method call
through a recording proxy (which engine, method, integer arguments, dtype and numel of every tensor argument).  What RCCL pairs up is
the order within a batch: a change of that order shows here and nowhere else on a box where RCCL cannot run two ranks."""
import argparse
import hashlib
import json
import os
import socket
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
BIG = dict(n_reads=3000, n_loci=300, n_haps=4, paired=True)
TINY = dict(n_reads=3, n_loci=50, n_haps=2)          # 4 ranks over 3 reads: empty shards, empty key ranges, skipped sends
CASES = tuple((world, BIG, protocol, None) for world in (2, 3) for protocol in ("ranges", "finalize_ranges", "root")) + \
    tuple((world, BIG, protocol, "multisample") for world in (2, 3) for protocol in ("ranges", "finalize_ranges")) + \
    tuple((4, TINY, protocol, None) for protocol in ("ranges", "finalize_ranges"))
COLLECTIVES = ("all_gather_into_tensor", "broadcast", "all_reduce")


def case_name(world, spec, protocol, after):
    return "world %d, %d reads, %s%s" % (world, spec["n_reads"], protocol, " + " + after if after else "")


def describe(a):
    """ints as they are, tensors as [dtype, numel], lists and tuples item by item."""
    if hasattr(a, "numel"):
        return [str(a.dtype), a.numel()]
    if isinstance(a, (list, tuple)):
        return [describe(x) for x in a]
    return a if a is None or isinstance(a, (bool, int)) else type(a).__name__


class Recorded(object):
    """An engine whose every method call goes into ``log`` first."""

    def __init__(self, inner, label, log):
        self._inner, self._label, self._log = inner, label, log
        self.device = inner.device

    def __getattr__(self, name):
        fn = getattr(self._inner, name)

        def call(*a):
            self._log.append(["engine", self._label, name, describe(a)])
            return fn(*a)
        return call


def record_dist(tdist, log):
    """Puts recorders in front of the ``torch.distributed`` calls the protocol makes -> what to call to take them away again."""
    saved = {n: getattr(tdist, n) for n in COLLECTIVES + ("batch_isend_irecv",)}

    def collective(name):
        def f(*a, **k):
            t = a[1] if name == "all_gather_into_tensor" else a[0]        # (what this rank puts in)
            extra = {"src": k.get("src")} if name == "broadcast" else {"op": str(k.get("op", "SUM"))} if name == "all_reduce" else {}
            log.append(["dist", name, str(t.dtype), t.numel(), extra])
            return saved[name](*a, **k)
        return f

    def batch(ops):
        log.append(["dist", "batch_isend_irecv", [[op.op.__name__, op.peer, str(op.tensor.dtype), op.tensor.numel()] for op in ops]])
        return saved["batch_isend_irecv"](ops)
    for n in COLLECTIVES:
        setattr(tdist, n, collective(n))
    tdist.batch_isend_irecv = batch
    return lambda: [setattr(tdist, n, f) for n, f in saved.items()]


def use_tree(tree):
    for p in (os.path.join(HERE, "..", "tests"), os.path.abspath(tree)):
        sys.path.insert(0, p)


def _rank(rank, world, port, tree, spec_args, protocol, after, out_dir):
    use_tree(tree)
    import torch.distributed as tdist
    from alntools_amd import dist as ecdist, synth
    assert os.path.abspath(ecdist.__file__).startswith(os.path.abspath(tree)), ecdist.__file__
    import test_dist_gloo as tg
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    tdist.init_process_group("gloo", rank=rank, world_size=world)
    spec = synth.SynthSpec(**spec_args)
    R = spec.n_reads
    a, b = rank * R // world, (rank + 1) * R // world
    inner = tg.OracleEngine(spec.n_haps)
    inner.build(synth.generate(spec, a, b))
    if after:
        base = synth.generate(spec, 0, a)["n_reads"] if a else 0
        inner.meta = [tg._meta_of(base + i) for i in range(inner.n_reads)]
    log = []
    eng = Recorded(inner, "shard", log)
    fresh = lambda label: (lambda: Recorded(tg.OracleEngine(spec.n_haps), label, log))
    undo = record_dist(tdist, log)
    try:
        if protocol == "root":
            merged = ecdist.exchange_and_merge_on_root(eng, fresh("root"), root=0)
        else:
            merged = ecdist.exchange_and_merge(eng, fresh("part"), fresh("root"), root=0, finalize_ranges=protocol == "finalize_ranges")
        assert (merged is None) == (rank != 0)
        log.append(["returned", None if merged is None else merged._label])
        if after:
            n_ecs = (len(merged._inner.csr()["indptr"]) - 1) if rank == 0 else None
            n = ecdist.exchange_multisample(eng, merged, n_ecs, root=0)
            log.append(["returned", n])
    finally:
        undo()
    with open(os.path.join(out_dir, "rank%d.json" % rank), "w") as fh:
        json.dump(log, fh)
    tdist.barrier()
    tdist.destroy_process_group()


def run_case(tree, world, spec_args, protocol, after):
    """-> the trace of every rank, in rank order."""
    import torch.multiprocessing as mp
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    with tempfile.TemporaryDirectory() as td:
        mp.spawn(_rank, args=(world, port, os.path.abspath(tree), spec_args, protocol, after, td), nprocs=world, join=True)
        return [json.load(open(os.path.join(td, "rank%d.json" % r))) for r in range(world)]


def canonical(trace):
    return json.dumps(trace, sort_keys=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.join(HERE, ".."))
    ap.add_argument("--out", default=None, help="the traces themselves, as JSON: {case: [trace of rank 0, ...]}")
    a = ap.parse_args()
    traces = {}
    for case in CASES:
        traces[case_name(*case)] = t = run_case(a.tree, *case)
        print("%-52s %4d events  %s" % (case_name(*case), sum(len(r) for r in t), hashlib.sha256(canonical(t).encode()).hexdigest()))
    print("%-52s %4d events  %s" % ("all cases", sum(len(r) for t in traces.values() for r in t), hashlib.sha256(canonical(traces).encode()).hexdigest()))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("{\n" + ",\n".join("%s: [\n%s\n]" % (json.dumps(k), ",\n".join(json.dumps(r) for r in t)) for k, t in traces.items()) + "\n}\n")
