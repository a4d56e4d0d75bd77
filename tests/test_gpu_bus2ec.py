"""bus2ec on the GPU.  (1) BUS directories made from the golden ``.bin`` files the reference wrote (``bus_checker.bus_from_bin``) must convert
back to them byte for byte through the command line -- plain, with every third read split over two wider ECs, shuffled and tripled, and
without UMIs; (2) seeded random inputs against the checker, exactly, at every size where the kernels change path (the constants come from
``test_bus_constants.py``); (3) one rule for every route; (4) every device-side refusal; (6) ``ecquant-cells`` on the result.

All shapes stay at or below 20 000 records, a few hundred targets and a few thousand target ids in ``matrix.ec``."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from alntools_amd import bin_utils, bus_utils, ecb, ecb_bus

import bus_checker as bc
from test_bus_constants import BUS_MERGE_LEN, BUS_WAVE_WORK, MAX_UMILEN, RS_TILE, SCB, TPB

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ARG, LIMIT, CONTRACT = -1, -8, -5             # include/ecb.h: ECB_ERR_ARG, ECB_ERR_LIMIT, ECB_ERR_CONTRACT
_kept = {}


def _u32(a):
    return np.asarray(a, dtype=np.uint32)


def _np(x):
    if hasattr(x, "cpu"):
        x = x.cpu().numpy()
    return np.asarray(x)


def _library(rec, bclen, umilen, lines, tcol, thap, n_loci, n_haps, keep=None, no_umi=False, tensors=False):
    ptr, ids = bc.csr_lines(lines)
    kp = None if keep is None else np.array(sorted(keep), dtype=np.uint64)
    if tensors:
        import torch
        rec = torch.as_tensor(np.ascontiguousarray(rec), device="cuda")
    b, A, N, rl, sizes = ecb_bus.molecules(rec, bclen, umilen, ptr, ids, _u32(tcol), _u32(thap), n_loci, n_haps, keep=kp, no_umi=no_umi)
    return _np(b).view(np.uint64), tuple(_np(x) for x in A), tuple(_np(x) for x in N), _np(rl), sizes


def _exact(rec, bclen, umilen, lines, tcol, thap, n_loci, n_haps, keep=None, no_umi=False, tensors=False):
    """The library's eight outputs against the checker's, exactly; -> the checker's result."""
    want = bc.molecules(rec, lines, tcol, thap, keep=keep, no_umi=no_umi)
    b, A, N, rl, sizes = _library(rec, bclen, umilen, lines, tcol, thap, n_loci, n_haps, keep, no_umi, tensors)
    assert sizes == want.sizes
    assert b.tolist() == want.barcodes and rl.tolist() == want.row_line
    for got, exp, what in zip(A + N, bc.csr(want.rows) + bc.csc(want.N, len(want.barcodes)), ("ipA", "ixA", "daA", "ipN", "ixN", "daN")):
        assert got.dtype == np.int32 and np.array_equal(got, exp), what
    return want


def _finish(lib, n_loci, n_haps, mincount):
    """``bus_utils``' second half on the library's outputs: ``ecb.combine`` as one part, then ``ecb.select``."""
    b, A, N, _rl, _sizes = lib
    part = dict(indptrA=A[0], indicesA=A[1], dataA=A[2], indptrN=N[0], indicesN=N[1], dataN=N[2], n_loci=n_loci, target_map=None,
                sample_map=np.arange(len(b), dtype=np.uint32))
    A_N, kept = ecb.select(*ecb.combine([part], n_loci, n_haps, len(b)), n_loci, n_haps, row_class=0, min_count=mincount)
    return A_N, kept


# ---- 1. the reference's bytes ---------------------------------------------------------------------------------------------------------------
def _cli_env():
    env = dict(os.environ)
    env.pop("ALNTOOLS_GPUS", None)
    env.pop("ALNTOOLS_TORCH", None)
    return env


GOLD = {"g4b": ("g4b_multi_min0.bin", {0: "g4b_multi_min0.bin", 40: "g4b_multi_min40.bin", 160: "g4b_multi_min160.bin"}),
        "g4": ("g4_multi_min0.bin", {20: "g4_multi_min20.bin", 60: "g4_multi_min60.bin"})}
VARIANTS = {"plain": {}, "split": dict(split=True), "shuffled-tripled": dict(split=True, shuffle=True, triple=True), "no-umi": dict(no_umi=True)}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("which", list(GOLD))
def test_a_golden_bin_as_a_bus_directory_converts_back_byte_for_byte(tmp_path, which, variant):
    source, wants = GOLD[which]
    m = bin_utils.ecload(os.path.join(GOLDEN, source))
    b = bc.bus_from_bin(m, str(tmp_path / "bus"), seed=11, **VARIANTS[variant])
    if which == "g4b" and variant == "plain":
        assert (m.num_reads, m.num_samples, int(m.dataN.sum())) == (845, 338, 20355) and len(b["records"]) == 20355
    assert not np.array_equal(b["values"], np.sort(b["values"]))                       # (the barcodes are not in sample order)
    for k, (mincount, golden) in enumerate(sorted(wants.items())):
        out = str(tmp_path / ("m%d.bin" % mincount))
        argv = [b["dir"], out, "-m", str(mincount), "--names", b["names"], "-l", b["lengths"]] + (["--no-umi"] if variant == "no-umi" else [])
        r = subprocess.run([sys.executable] + (["-X", "importtime"] if k == 0 else []) + ["-m", "alntools_amd.cli", "bus2ec"] + argv, cwd=ROOT,
                           env=_cli_env(), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        if k == 0:
            imported = [l.split("|")[-1].strip() for l in r.stderr.splitlines() if l.startswith("import time:")]
            assert "alntools_amd.ecb_bus" in imported and not any(x == "torch" or x.startswith("torch.") for x in imported)
        with open(out, "rb") as got, open(os.path.join(GOLDEN, golden), "rb") as want:
            assert got.read() == want.read(), (which, variant, mincount)


def test_a_keep_list_that_names_no_barcode_of_the_file_is_refused(tmp_path):
    m = bin_utils.ecload(os.path.join(GOLDEN, "g4_multi_min0.bin"))
    b = bc.bus_from_bin(m, str(tmp_path / "bus"), seed=11)
    names = str(tmp_path / "none.txt")
    with open(names, "w") as fh:
        fh.write("%s\tnobody\n%s\tnobody2\n" % ("ACGT" * 4, "TTTT" * 4))
    out = str(tmp_path / "out.bin")
    r = subprocess.run([sys.executable, "-m", "alntools_amd.cli", "bus2ec", b["dir"], out, "--names", names], cwd=ROOT, env=_cli_env(),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "Error: no sample left" in r.stderr and not os.path.exists(out)
    r = subprocess.run([sys.executable, "-m", "alntools_amd.cli", "bus2ec", b["dir"], out, "-m", "100000"], cwd=ROOT, env=_cli_env(),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "Error: no sample left" in r.stderr and not os.path.exists(out)


# ---- 2. against the checker, exactly ----------------------------------------------------------------------------------------------------------
T, H = 240, 2
TCOL, THAP = (np.arange(T) // H).tolist(), (np.arange(T) % H).tolist()


def _lines(rng, n_lines=60, longest=12):
    """Random lines over a common core, so that intersections are often not empty, and one line holding every target."""
    core = sorted(rng.choice(T, size=4, replace=False).tolist())
    out = []
    for _ in range(n_lines):
        extra = rng.choice(T, size=int(rng.integers(0, longest)), replace=False).tolist()
        out.append(sorted(set(extra) | set(c for c in core if rng.random() < 0.8)) or [int(rng.integers(T))])
    return out + [list(range(T))]


def _random_records(rng, n, n_cells, n_umis, n_lines, bclen=16, umilen=8):
    bcs = rng.choice(1 << min(2 * bclen, 40), size=n_cells, replace=False).astype(np.uint64)
    return bc.records(bcs[rng.integers(0, n_cells, size=n)], rng.integers(0, n_umis, size=n).astype(np.uint64), rng.integers(0, n_lines, size=n),
                      rng.integers(0, 4, size=n))


EDGES = [e + d for e in (TPB, RS_TILE, SCB) for d in (-1, 0, 1)]


@pytest.mark.parametrize("n", EDGES)
def test_molecules_across_a_thread_workgroup_and_tile_edge(n):
    """Molecules of three and four records in two cells: whatever n is, one straddles every multiple of the workgroup, the sort tile and the
    scan's stretch in the sorted order; n itself sits one below, on and one above each."""
    rng = np.random.default_rng(n)
    lines = _lines(rng)
    j = np.arange(n)
    rec = bc.records((np.uint64(3) + (j % 2).astype(np.uint64) * np.uint64(1 << 20)), (j // 7).astype(np.uint64), rng.integers(0, len(lines), size=n), 1)
    rec = rec[rng.permutation(n)]
    want = _exact(rec, 16, 8, lines, TCOL, THAP, T // H, H)
    assert want.sizes[0] == 2 and want.sizes[5] > n // 16
    _exact(rec, 16, 8, lines, TCOL, THAP, T // H, H, no_umi=True)


def test_molecules_of_k_ecs():
    """k = 1, 2, 3, 63, 64, 65 and 300 distinct ECs in one molecule, every line {0, j + 1}: the candidate list has 2 targets, so k - 1 = 63 is
    below BUS_WAVE_WORK = 128 = 2 x 64 (a lane's) and k = 65 on it (a wave's); the intersection is {0} every time."""
    assert BUS_WAVE_WORK == 128
    ks = [1, 2, 3, 63, 64, 65, 300]
    lines = [[0, j + 1] for j in range(400)]
    bcs, umis, ecs = [], [], []
    rng = np.random.default_rng(1)
    for u, k in enumerate(ks):
        for e in rng.choice(400, size=k, replace=False):
            bcs.append(5); umis.append(u); ecs.append(int(e))
            if k > 3 and e % 5 == 0:                                # (some ECs twice in the molecule)
                bcs.append(5); umis.append(u); ecs.append(int(e))
    rec = bc.records(np.array(bcs, dtype=np.uint64), np.array(umis, dtype=np.uint64), ecs, 1)
    tcol, thap = np.arange(401).tolist(), [0] * 401
    want = _exact(rec[np.random.default_rng(2).permutation(len(rec))], 16, 8, lines, tcol, thap, 401, 1)
    assert want.sizes[4:] == (7, 6, 0, 6) and all(r == ((0,), (1,)) for r in want.rows[1:])


@pytest.mark.parametrize("clen", sorted(set([BUS_MERGE_LEN - 1, BUS_MERGE_LEN, BUS_MERGE_LEN + 1, 63, 64, 65, BUS_WAVE_WORK // 2 - 1, BUS_WAVE_WORK // 2,
                                             BUS_WAVE_WORK // 2 + 1, BUS_WAVE_WORK - 1, BUS_WAVE_WORK, BUS_WAVE_WORK + 1])))
def test_intersections_on_both_sides_of_every_path_switch(clen):
    """A candidate list of ``clen`` targets against: the line of every target (the intersection is a matrix.ec line), a longer line that
    holds some of them (bisected), a short one (walked, BUS_MERGE_LEN on both sides), both (k = 3: clen x 2 crosses BUS_WAVE_WORK at half
    the length), and a line that shares nothing (empty)."""
    rng = np.random.default_rng(clen)
    every = list(range(T))
    a = sorted(rng.choice(T, size=clen, replace=False).tolist())
    rest = [t for t in every if t not in set(a)]
    longer = sorted(a[::2] + rest[:clen + 3])
    lines = [a, every, longer, sorted(a[:3] + rest[:BUS_MERGE_LEN - 3]), sorted(a[:3] + rest[:BUS_MERGE_LEN - 2]), rest[:max(clen, 1)], a[1:2]]
    mols = [(0, 1), (0, 2), (0, 3), (0, 4), (0, 1, 2), (0, 2, 3), (0, 5), (0,), (1,), (0, 6), (1, 2), (5, 6)]
    bcs, umis, ecs = [], [], []
    for u, es in enumerate(mols):
        for cellno in (7, 9):
            for e in es:
                bcs.append(cellno); umis.append(u); ecs.append(e)
    rec = bc.records(np.array(bcs, dtype=np.uint64), np.array(umis, dtype=np.uint64), ecs, 1)
    want = _exact(rec, 16, 8, lines, TCOL, THAP, T // H, H)
    assert want.sizes[6] == 4 and want.sizes[7] == 2 * (len(mols) - 4)


def test_intersections_equal_to_a_line_to_each_other_and_only_after_the_mapping():
    """Targets 0 and 3 share (column 0, haplotype 0) and never meet in a row: the intersections {0} and {3} are different target sets and the
    same EC.  Fifty molecules found the row {0}, which is line 4's and gets a read of its own; two are empty; one founds the EC {1}.  The
    checker's whole rule against combine + select."""
    tcol, thap = [0, 1, 2, 0, 1, 2], [0, 0, 0, 0, 1, 1]
    lines = [[0, 1], [0, 2], [3, 4], [3, 5], [0], [1, 2], [1, 4]]
    mols = [((c, u), (0, 1)) for c in range(5) for u in range(10)] + [((1, 20), (2, 3)), ((2, 21), (0, 4)), ((2, 22), (4,)), ((3, 23), (1, 2)),
                                                                   ((4, 24), (0, 1, 5)), ((3, 25), (5, 6))]
    bcs, umis, ecs = zip(*[(c, u, e) for (c, u), es in mols for e in es])
    rec = bc.records(np.array(bcs, dtype=np.uint64), np.array(umis, dtype=np.uint64), ecs, 1)
    want = _exact(rec, 4, 4, lines, tcol, thap, 3, 2)
    assert want.sizes == (5, 54, 54, 54, 56, 55, 2, 53) and want.rows.count(((0,), (1,))) == 53
    lib = _library(rec, 4, 4, lines, tcol, thap, 3, 2)
    full = bc.bus2ec(rec, 4, lines, tcol, thap, mincount=11)
    assert full.samples == ["AAAC", "AAAG", "AAAT"] and full.stats["new_ecs"] == 1         # (the first and the last cell count 10 molecules: they go)
    A_N, kept = _finish(lib, 3, 2, 11)
    assert kept.tolist() == [False, True, True, True, False]
    for got, exp in zip(A_N, full.A + full.N):
        assert np.array_equal(got, exp)


def test_umi_zero_and_all_ones():
    """UMI 0 and the all-ones UMI of the longest supported length, in neighbouring cells: the last molecule of one cell and the first of the
    next differ in the cell bits alone."""
    ones = (1 << (2 * MAX_UMILEN)) - 1
    lines = [[0, 1], [1, 2], [2]]
    rows = [(1, 0, 0), (1, 0, 1), (1, ones, 0), (1, ones, 1), (2, 0, 1), (2, 0, 2), (2, ones, 2), (3, ones, 0), (3, 0, 0), (3, ones - 1, 1), (3, ones - 1, 0)]
    rec = bc.records(*[np.array([r[k] for r in rows], dtype=np.uint64 if k < 2 else np.int64) for k in range(3)], 1)
    want = _exact(rec, 16, MAX_UMILEN, lines, [0, 1, 2], [0, 0, 0], 3, 1)
    assert want.sizes[4:] == (7, 4, 0, 4)
    with pytest.raises(ecb.EcbError) as e:
        _library(rec, 16, MAX_UMILEN + 1, lines, [0, 1, 2], [0, 0, 0], 3, 1)
    assert e.value.code == LIMIT
    _exact(rec, 16, 32, lines, [0, 1, 2], [0, 0, 0], 3, 1, no_umi=True)


@pytest.mark.parametrize("bclen", [16, 17, 32])
def test_barcode_lengths(bclen):
    rng = np.random.default_rng(bclen)
    lines = _lines(rng)
    n = 3000
    top = (1 << (2 * bclen)) - 1
    bcs = np.array([0, 1, top, top - 1, top >> 1, (top >> 1) + 1, 1 << 32, (1 << 32) - 1][:8 if bclen > 16 else 6], dtype=np.uint64)
    bcs = np.unique(np.minimum(bcs, np.uint64(top)))
    rec = bc.records(bcs[rng.integers(0, len(bcs), size=n)], rng.integers(0, 300, size=n).astype(np.uint64), rng.integers(0, len(lines), size=n),
                     rng.integers(0, 3, size=n))
    want = _exact(rec, bclen, 8, lines, TCOL, THAP, T // H, H)
    assert want.barcodes == sorted(bcs.tolist()) and (bclen < 32 or want.barcodes[-1] >> 63)
    _exact(rec, bclen, 8, lines, TCOL, THAP, T // H, H, keep=[int(bcs[-1]), int(bcs[0]), 12345], no_umi=True)


@pytest.mark.parametrize("shape", ["one-cell", "a-cell-per-record"])
@pytest.mark.parametrize("no_umi", [False, True])
def test_one_cell_and_a_cell_per_record(shape, no_umi):
    rng = np.random.default_rng(len(shape))
    lines = _lines(rng)
    n = 2500
    rec = _random_records(rng, n, 1 if shape == "one-cell" else n, 100, len(lines))
    if shape != "one-cell":
        rec = bc.records(rng.permutation(n).astype(np.uint64) * np.uint64(3), *bc.fields(rec)[1:])
    want = _exact(rec, 16, 8, lines, TCOL, THAP, T // H, H, no_umi=no_umi)
    assert want.sizes[0] == (1 if shape == "one-cell" else n)


@pytest.mark.parametrize("no_umi", [False, True])
@pytest.mark.parametrize("keep", [None, "half", "none"])
def test_random_directories_with_and_without_a_keep_list(tmp_path, keep, no_umi):
    """The whole command in-process against the checker's whole rule: A, N, the sample names and ``--stats``."""
    rng = np.random.default_rng(7)
    lines = _lines(rng, n_lines=120)
    rec = _random_records(rng, 20000, 40, 400, len(lines))
    cells = sorted(set(bc.fields(rec)[0]))
    listed = None
    if keep == "half":
        listed = [(b, "cell%d" % k) for k, b in enumerate(cells[::2])][::-1] + [(3, "absent")]
    elif keep == "none":
        listed = [(3, "absent"), (4, "absent2")]
    lib_keep = None if listed is None else [b for b, _ in listed]
    want = _exact(rec, 16, 8, lines, TCOL, THAP, T // H, H, keep=lib_keep, no_umi=no_umi)
    if keep != "none":
        assert want.sizes[5] > 1000 or no_umi
        assert no_umi or (want.sizes[6] > 10 and want.sizes[7] > 100)
    names = ["t%d_%s" % (t // H, "AB"[t % H]) for t in range(T)]
    d = bc.write_bus_dir(str(tmp_path / "bus"), rec, 16, 8, lines, names)
    nf = None
    if listed is not None:
        nf = str(tmp_path / "names.txt")
        with open(nf, "w") as fh:
            fh.write("".join("%s\t%s\n" % (bc.decode(b, 16), n) for b, n in listed))
    out, stats = str(tmp_path / "out.bin"), str(tmp_path / "stats.txt")
    if keep == "none":
        with pytest.raises(ValueError, match="no sample left"):
            bus_utils.convert(d, out, no_umi=no_umi, mincount=0, names_file=nf, stats_file=stats)
        assert not os.path.exists(out) and not os.path.exists(stats)
        return
    mincount = 300 if keep is None else 0
    bus_utils.convert(d, out, no_umi=no_umi, mincount=mincount, names_file=nf, stats_file=stats)
    full = bc.bus2ec(rec, 16, lines, TCOL, THAP, names=listed, mincount=mincount, no_umi=no_umi)
    m = bin_utils.ecload(out)
    assert m.sname == full.samples and m.lname == ["t%d" % t for t in range(T // H)] and m.hname == ["A", "B"] and not m.lengths.any()
    for got, exp in zip((m.indptrA, m.indicesA, m.dataA, m.indptrN, m.indicesN, m.dataN), full.A + full.N):
        assert np.array_equal(got, exp)
    assert open(stats).read() == bus_utils.stats_text(full.stats)
    assert keep is not None or 0 < full.stats["cells_kept"] < full.stats["cells"] or no_umi


# ---- 3. one rule for every route --------------------------------------------------------------------------------------------------------------
def _route_input():
    rng = np.random.default_rng(21)
    lines = _lines(rng, n_lines=100)
    return _random_records(rng, 3 * RS_TILE + 5, 30, 500, len(lines)), lines


def _digest(out):
    b, A, N, rl, sizes = out
    h = hashlib.sha256()
    for x in (b,) + A + N + (rl, np.array(sizes, dtype=np.uint64)):
        h.update(np.ascontiguousarray(x).tobytes())
    return h.hexdigest()


def _routes():
    rec, lines = _route_input()
    keep = sorted(set(bc.fields(rec)[0]))[3:]
    return [_digest(_library(rec, 16, 8, lines, TCOL, THAP, T // H, H, keep=kp, no_umi=nu, tensors=tensors))
            for tensors in (False, True) for kp in (None, keep) for nu in (False, True)]


def test_the_host_entry_the_device_entry_and_a_second_call_give_the_same_bytes():
    first, second = _routes(), _routes()
    assert first[:4] == first[4:] and first == second and len(set(first)) == 4
    _kept["routes"] = first
    rec, lines = _route_input()
    _exact(rec, 16, 8, lines, TCOL, THAP, T // H, H)


def test_everything_once_more_with_the_scratch_poisoned_gives_the_same_bytes():
    if "routes" not in _kept:
        _kept["routes"] = _routes()
    env = dict(os.environ)
    env["ECB_POISON_SCRATCH"] = "1"
    env["ALNTOOLS_TORCH"] = "1"
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_bus2ec as t; print('digest', ' '.join(t._routes() + t._routes()))"
            % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "digest " + " ".join(_kept["routes"] * 2) in r.stdout


# ---- 4. the device-side refusals --------------------------------------------------------------------------------------------------------------
PATTERN = 0x5C


class _Raw(object):
    """``ecb_bus_molecules_device`` called by hand: inputs as CUDA tensors, outputs pre-filled with 0x5C at exactly the capacities."""

    def __init__(self, rec, lines, bclen=16, umilen=8):
        import torch
        self.torch, self.lib = torch, ecb_bus.load()
        self.rec = np.ascontiguousarray(rec).reshape(-1, 32)
        self.ptr, self.ids = bc.csr_lines(lines)
        self.bclen, self.umilen = bclen, umilen
        self.n = len(self.rec)
        self.caps = (self.n, self.n, ecb_bus.a_capacity(self.rec, self.ptr), self.n)

    def call(self, rec=None, flags=0, caps=None, bclen=None, umilen=None):
        torch = self.torch
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy(), device="cuda")
        cc, cr, ca, cn = self.caps if caps is None else caps
        ins = [dev(self.rec if rec is None else rec), dev(self.ptr), dev(self.ids), dev(_u32(TCOL)), dev(_u32(THAP))]
        self.outs = [torch.full((max(nb, 1),), PATTERN, dtype=torch.uint8, device="cuda")
                     for nb in (cc * 8, (cr + 1) * 4, ca * 4, ca * 4, (cc + 1) * 4, cn * 4, cn * 4, cr * 4)]
        sizes = (C.c_uint64 * 8)(*[7] * 8)
        P = ecb._dev_ptr
        rc = self.lib.ecb_bus_molecules_device(0, P(ins[0]), self.n, self.bclen if bclen is None else bclen, self.umilen if umilen is None else umilen,
                                               flags, len(self.ptr) - 1, len(self.ids), P(ins[1]), P(ins[2]), T, P(ins[3]), P(ins[4]), T // H, H, None, 0,
                                               cc, cr, ca, cn, *([P(o) for o in self.outs] + [sizes]))
        torch.cuda.synchronize()
        return rc, tuple(sizes), (self.lib.ecb_last_error(None) or b"").decode()

    def untouched(self):
        return all(bool((o == PATTERN).all()) for o in self.outs)


def _raw_case():
    def make():
        rng = np.random.default_rng(33)
        lines = _lines(rng)
        rec = _random_records(rng, 2 * TPB + 9, 6, 60, len(lines))
        raw = _Raw(rec, lines)
        rc, sizes, msg = raw.call()
        assert rc == 0, msg
        assert sizes == bc.molecules(rec, lines, TCOL, THAP).sizes
        return raw, lines, sizes
    if "raw" not in _kept:
        _kept["raw"] = make()
    return _kept["raw"]


def _refused(raw, good, code, text, **kw):
    rc, sizes, msg = raw.call(**kw)
    assert rc == code and text in msg, (rc, msg)
    assert sizes == (7,) * 8 and raw.untouched()
    rc, sizes, msg = raw.call()
    assert rc == 0 and sizes == good, msg


def _with(rec, at, field, value):
    r = rec.copy().reshape(-1).view([("bc", "<u8"), ("umi", "<u8"), ("ec", "<i4"), ("count", "<u4"), ("flags", "<u4"), ("pad", "<u4")])
    for i in np.atleast_1d(at):
        r[field][i] = value
    return r.view(np.uint8).reshape(-1, 32)


@pytest.mark.parametrize("at", ["first", "middle", "last", "two"])
@pytest.mark.parametrize("value", ["below", "beyond"])
def test_an_ec_out_of_range_is_refused_with_the_lowest_record(at, value):
    raw, lines, good = _raw_case()
    where = {"first": [0], "middle": [raw.n // 2], "last": [raw.n - 1], "two": [raw.n - 3, TPB + 1]}[at]
    bad = _with(raw.rec, where, "ec", -1 if value == "below" else len(lines))
    _refused(raw, good, CONTRACT, "bus: record %d: ec below 0 or at or beyond" % min(where), rec=bad)


def test_a_barcode_or_umi_bit_too_high_is_refused():
    raw, lines, good = _raw_case()
    _refused(raw, good, CONTRACT, "bus: record 70: a barcode bit", rec=_with(raw.rec, [300, 70], "bc", 1 << 32))
    _refused(raw, good, CONTRACT, "bus: record 5: a UMI bit", rec=_with(raw.rec, 5, "umi", 1 << 16))
    _refused(raw, good, CONTRACT, "bus: record 5: a UMI bit", rec=_with(raw.rec, 5, "umi", 1 << 16), flags=ecb_bus.NO_UMI)
    _refused(raw, good, CONTRACT, "bus: record 9: a barcode bit", rec=_with(_with(raw.rec, 11, "umi", 1 << 63), 9, "bc", 1 << 63))
    # flags and pad are ignored
    rc, sizes, msg = raw.call(rec=_with(_with(raw.rec, [0, 5], "flags", 0xFFFFFFFF), [1, 6], "pad", 0xDEADBEEF))
    assert rc == 0 and sizes == good, msg


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_a_capacity_one_too_small_is_refused_and_the_exact_one_is_enough(which):
    raw, lines, good = _raw_case()
    exact = list(good[:4])
    rc, sizes, msg = raw.call(caps=exact)
    assert rc == 0 and sizes == good, msg
    short = list(exact)
    short[which] -= 1
    _refused(raw, good, ARG, "room for", caps=short)


def test_a_count_beyond_int32_is_refused():
    raw, lines, good = _raw_case()
    bcs, _, ecs, _ = bc.fields(raw.rec)
    b0, e0 = bcs[0], ecs[0]
    same = [i for i in range(raw.n) if bcs[i] == b0 and ecs[i] == e0]                   # (every other record of that row and cell counts nothing)
    rec = _with(_with(_with(raw.rec, [3, 4], "bc", b0), [3, 4], "ec", e0), same + [3, 4], "count", 0)
    rec = _with(_with(rec, 3, "count", 0x7FFFFFFF), 4, "count", 1)                      # (2^31 - 1) + 1 in one (row, cell)
    _refused(raw, good, LIMIT, "beyond int32", rec=rec, flags=ecb_bus.NO_UMI)
    rc, sizes, msg = raw.call(rec=_with(rec, 4, "count", 0), flags=ecb_bus.NO_UMI)      # 2^31 - 1 fits
    assert rc == 0, msg
    rc, sizes, msg = raw.call(rec=rec)                                                  # with UMIs the counts are ignored
    assert rc == 0, msg


def test_the_command_names_the_file_and_the_record_of_a_device_side_refusal(tmp_path):
    raw, lines, good = _raw_case()
    names = ["t%d_%s" % (t // H, "AB"[t % H]) for t in range(T)]
    out = str(tmp_path / "out.bin")
    for k, (rec, text, kw) in enumerate((
            (_with(raw.rec, [400, 90], "ec", len(lines)), "output.bus record 90: ec below 0 or at or beyond the number of matrix.ec lines", {}),
            (_with(raw.rec, 17, "bc", 1 << 32), "output.bus record 17: a barcode bit at or above 2 x bclen", {}),
            (_with(raw.rec, 2, "umi", 1 << 16), "output.bus record 2: a UMI bit at or above 2 x umilen", dict(no_umi=True)),
            (_with(_with(raw.rec, [3, 4], "bc", 5), [3, 4], "ec", 0), "beyond int32", dict(no_umi=True)))):
        if text == "beyond int32":
            rec = _with(rec, [3, 4], "count", 0x7FFFFFFF)
        d = bc.write_bus_dir(str(tmp_path / ("bus%d" % k)), rec, 16, 8, lines, names)
        with pytest.raises(ValueError) as e:
            bus_utils.convert(d, out, mincount=0, **kw)
        assert text in str(e.value) and str(e.value).count("record") <= 1 and not os.path.exists(out), str(e.value)


def test_bad_arguments_are_refused_before_anything_runs():
    raw, lines, good = _raw_case()
    for kw, code in ((dict(bclen=0), ARG), (dict(bclen=33), ARG), (dict(umilen=0), ARG), (dict(umilen=33), ARG), (dict(flags=2), ARG),
                     (dict(umilen=MAX_UMILEN + 1), LIMIT)):
        _refused(raw, good, code, "bus: ", **kw)


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------------------
def test_ecquant_cells_on_the_converted_file_equals_ecquant_cells_on_the_golden_file(tmp_path):
    golden = os.path.join(GOLDEN, "g4_multi_min20.bin")
    b = bc.bus_from_bin(bin_utils.ecload(os.path.join(GOLDEN, "g4_multi_min0.bin")), str(tmp_path / "bus"), seed=2, split=True, shuffle=True)
    out = str(tmp_path / "converted.bin")
    bus_utils.convert(b["dir"], out, mincount=20, names_file=b["names"], lengths_file=b["lengths"])
    tables = []
    for k, f in enumerate((out, golden)):
        table = str(tmp_path / ("cells%d.tsv" % k))
        bin_utils.ecquant_cells(f, table, use_lengths=True, max_iters=50)
        with open(table, "rb") as fh:
            tables.append(fh.read())
    assert tables[0] == tables[1] and len(tables[0]) > 1000
