"""ecdownsample on the GPU (``ecb_downsample`` / ``ecb_downsample_device``) against the checker (``tests/downsample_checker.py``), exactly:
the golden files through the binding, ``bin_utils`` and the command line under each rule, every size of a sample around the two paths'
thresholds with every kind of target, every shape of a column, entry and sample boundaries on either side of every thread's, wave's and
workgroup's stretch of reads, the searched cases whose select goes into the key's second word, one rule for every route (host and device
entry, a second call, the scratch poisoned, whatever the other samples' targets are) and every refusal with its outputs untouched.
Digits beyond the fifth cannot be reached with real keys at any size a test can run: ``test_ecdownsample.py``'s host program covers them."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from alntools_amd import bin_utils, ecb, ecb_downsample as ed

import downsample_checker as dc
from test_downsample_constants import SMALL, THREAD, WAVE, WG
from test_ecdownsample import SECOND_WORD

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = ("g4b_multi_min0.bin", "g4_multi_min0.bin")
ARG, CONTRACT, LIMIT = -1, -5, -8             # include/ecb.h: ECB_ERR_ARG, ECB_ERR_CONTRACT, ECB_ERR_LIMIT
_loaded = {}


def _bytes(p):
    with open(p, "rb") as f:
        return f.read()


def _load(name):
    if name not in _loaded:
        _loaded[name] = bin_utils.ecload(os.path.join(GOLDEN, name))
    return _loaded[name]


def _agree(ptr, ec, cnt, n_ecs, target, seed=0, tensors=False, want=None):
    """The library's three outputs are the checker's, exactly -> them."""
    want = want or dc.downsample(ptr, ec, cnt, n_ecs, target, seed)
    a = [np.asarray(x, dtype=np.int32) for x in (ptr, ec, cnt)] + [np.asarray(target, dtype=np.int64)]
    if tensors:
        import torch
        a = [torch.as_tensor(x, device="cuda") for x in a]
    got = ed.downsample(a[0], a[1], a[2], n_ecs, a[3], seed=seed)
    if tensors:
        assert all(g.is_cuda for g in got)
        got = [g.cpu().numpy() for g in got]
    for g, w, name in zip(got, want, ("out_data_n", "in_total", "out_total")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (name, np.flatnonzero(np.asarray(g) != w)[:8])
    return want


def _split(rng, M, k):
    """M reads over k entries, every entry with at least one where M allows (k <= M)."""
    cuts = np.sort(rng.choice(np.arange(1, M), size=min(k, M) - 1, replace=False)) if M > 1 else np.zeros(0, dtype=np.int64)
    return np.diff(np.concatenate([[0], cuts, [M]])).astype(np.int64)


def _n_of(columns, n_ecs=None):
    """Columns of counts -> (indptr, EC indices ascending from 0 in every column, counts, n_ecs)."""
    ptr = np.concatenate([[0], np.cumsum([len(c) for c in columns])]).astype(np.int64)
    ec = np.concatenate([np.arange(len(c)) for c in columns] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    cnt = np.concatenate([np.asarray(c, dtype=np.int64) for c in columns] + [np.zeros(0, dtype=np.int64)])
    return ptr, ec, cnt, n_ecs or max(1, max(len(c) for c in columns))


# ---- 1. the golden files ----------------------------------------------------------------------------------------------------------------------
def _rule(m, rule):
    M = dc.totals(m)
    return {"reads": dict(reads=int(np.sort(M)[len(M) // 2])), "fraction": dict(fraction=0.37), "equalize": dict(equalize=True, mincount=int(np.sort(M)[len(M) // 3]))}[rule]


@pytest.mark.parametrize("rule", ["reads", "fraction", "equalize"])
@pytest.mark.parametrize("name", FILES)
def test_the_golden_files_through_the_binding_bin_utils_and_the_command_line(tmp_path, name, rule):
    m, src, out, stats = _load(name), os.path.join(GOLDEN, name), str(tmp_path / "o.bin"), str(tmp_path / "s.tsv")
    kw = _rule(m, rule)
    stay = dc.staying(m, None, kw.get("mincount"))
    target = dc.targets(m, stay, kw.get("reads"), kw.get("fraction"), kw.get("equalize", False))
    assert ((target >= 0) & (target < dc.totals(m))).any()                  # some sample is thinned
    for tensors in (False, True):
        _agree(m.indptrN, m.indicesN, m.dataN, m.num_reads, target, seed=5, tensors=tensors)
    exp, rows = dc.ecdownsample(m, seed=5, **kw)
    want = bin_utils.ecsave2_bytes(exp)
    bin_utils.ecdownsample(src, out, seed=5, stats_file=stats, **kw)
    assert _bytes(out) == want
    assert open(stats).read().splitlines()[1:] == ["\t".join(str(v) for v in r) for r in rows]
    os.remove(out)
    env = dict(os.environ)
    env.pop("ALNTOOLS_GPUS", None)
    env["ALNTOOLS_TORCH"] = "0"
    flags = {"reads": ["-n", str(kw.get("reads"))], "fraction": ["-f", "0.37"], "equalize": ["--equalize", "-m", str(kw.get("mincount"))]}[rule]
    r = subprocess.run([sys.executable, "-m", "alntools_amd.cli", "ecdownsample", src, out, "--seed", "5", "-v"] + flags, cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert _bytes(out) == want and "samples: {:,} (from {:,})".format(exp.num_samples, m.num_samples) in r.stderr


def test_reads_n_leaves_exactly_n_reads_to_count_and_the_cells_quantify(tmp_path):
    name = FILES[0]
    m, src, out, table = _load(name), os.path.join(GOLDEN, name), str(tmp_path / "o.bin"), str(tmp_path / "cells.tsv")
    M = dc.totals(m)
    n = int(np.sort(M)[len(M) // 2])
    bin_utils.ecdownsample(src, out, reads=n, seed=1, mincount=2)
    o = bin_utils.ecload(out)
    thinned = [k for k, s in enumerate(o.sname) if M[m.sname.index(s)] > n]
    assert len(thinned) > 3 and o.num_samples == int((M >= 2).sum())
    pop = np.zeros(o.num_reads, dtype=np.int64)                               # set bits per row of A
    np.add.at(pop, np.repeat(np.arange(o.num_reads), np.diff(o.indptrA)), [bin(int(d)).count("1") for d in o.dataA])
    for k in thinned[:2] + thinned[-1:]:
        a, b = int(o.indptrN[k]), int(o.indptrN[k + 1])
        w = np.zeros(o.num_reads, dtype=np.int64)
        np.add.at(w, o.indicesN[a:b], o.dataN[a:b])
        aln = ecb.count_alignments(o.indptrA, o.indicesA, o.dataA, o.num_loci, o.num_haplotypes, o.indptrN, o.indicesN, o.dataN, sample=k)[0]
        assert int(w.sum()) == n and int(aln.sum()) == int((w * pop).sum())    # the sample's weights add up to n, and they are what is counted
    assert dc.totals(o)[thinned].tolist() == [n] * len(thinned)
    bin_utils.ecquant_cells(out, table, max_iters=5)
    assert len(open(table).read().splitlines()) > o.num_samples


# ---- 2. the sizes of a sample -----------------------------------------------------------------------------------------------------------------
SIZES = [1, 2, SMALL - 1, SMALL, SMALL + 1, 2 * WG + 1]


@pytest.mark.parametrize("M", SIZES)
def test_sizes_of_a_sample(M):
    rng = np.random.default_rng(M)
    targets = [0, 1, M - 1, M, M + 1, -1]
    ptr, ec, cnt, E = _n_of([_split(rng, M, int(rng.integers(1, 40))) for _ in targets])
    _agree(ptr, ec, cnt, E, targets, seed=M)
    for n in targets:                                                       # ... and each alone, as sample 0
        _agree(*_n_of([_split(rng, M, 7)]), [n], seed=3)


# ---- 3. the shapes of a column ----------------------------------------------------------------------------------------------------------------
def _shape(what):
    rng = np.random.default_rng(len(what))
    if what == "one_entry_of_all_reads":
        return _n_of([[100000]]) + ([31337],)
    if what == "every_entry_of_count_1":
        return _n_of([np.ones(3 * WG + 5), np.ones(SMALL - 3)]) + ([WG, 100],)
    if what == "zero_counts_in_front_between_and_behind":
        small, large = [0, 0, 5, 0, 0, 0, 9, 1, 0], np.concatenate([np.zeros(300), _split(rng, 9000, 40), np.zeros(700), _split(rng, 5000, 3), np.zeros(260)])
        return _n_of([small, large, [0, 0, 0]]) + ([7, 6000, 2],)
    if what == "an_ec_listed_twice":
        ptr, ec, cnt, E = _n_of([[30, 40, 50, 60], _split(rng, 7000, 6)])
        ec[:4], ec[4:] = [2, 2, 0, 2], [1, 1, 1, 3, 3, 0]
        return ptr, ec, cnt, 4, [90, 3500]
    if what == "an_empty_column_between_two_full_ones":
        return _n_of([_split(rng, 3000, 30), [], _split(rng, 1000, 30)]) + ([1500, 0, 999],)
    if what == "a_large_sample_between_small_ones":
        return _n_of([_split(rng, 50, 9), _split(rng, 20000, 300), _split(rng, 2048, 100)]) + ([25, 10000, 1024],)
    if what == "a_small_sample_between_large_ones":
        return _n_of([_split(rng, 20000, 300), _split(rng, 50, 9), _split(rng, 2049, 100)]) + ([19999, 49, 1],)
    if what == "3000_samples_of_1_to_40_reads":
        cols = [_split(rng, int(M), int(rng.integers(1, 9))) for M in rng.integers(1, 41, 3000)]
        return _n_of(cols) + (rng.integers(-1, 42, 3000),)
    if what == "one_sample_of_2_to_the_20_reads":
        return _n_of([_split(rng, 1 << 20, 5000)]) + ([1 << 19],)
    raise KeyError(what)


SHAPES = ["one_entry_of_all_reads", "every_entry_of_count_1", "zero_counts_in_front_between_and_behind", "an_ec_listed_twice",
          "an_empty_column_between_two_full_ones", "a_large_sample_between_small_ones", "a_small_sample_between_large_ones",
          "3000_samples_of_1_to_40_reads", "one_sample_of_2_to_the_20_reads"]


@pytest.mark.parametrize("what", SHAPES)
def test_shapes_of_a_column(what):
    ptr, ec, cnt, E, target = _shape(what)
    tin, tout = _agree(ptr, ec, cnt, E, target, seed=11)[1:]
    assert (tout <= tin).all() and (tout < tin).any()


def _stretch_edges():
    """Read numbers on either side of every thread's, wave's and workgroup's stretch of a large sample's first three stretches."""
    at = set()
    for unit in (THREAD, WAVE, WG):
        for k in (1, 2, 3, WG // unit - 1, WG // unit, WG // unit + 1, 2 * WG // unit, 3 * WG // unit):
            at.update((k * unit - 1, k * unit, k * unit + 1))
    return sorted(a for a in at if 0 < a)


def test_boundaries_on_either_side_of_every_stretch():
    edges = _stretch_edges()
    M = 3 * WG + THREAD + 3
    inner = [e for e in edges if e < M]
    entries = np.diff(np.concatenate([[0], inner, [M]]))                    # entries that end at every edge
    assert len(inner) > 30 and (entries > 0).all()
    ends = [WG - 1, WG, WG + 1, 2 * WG - 1, 2 * WG, 2 * WG + 1, WG + WAVE - 1, WG + WAVE, WG + WAVE + 1, WG + THREAD - 1, WG + THREAD, WG + THREAD + 1,
            2 * WG + WAVE + THREAD + 1]                                     # samples that end at every kind of edge
    rng = np.random.default_rng(4)
    cols = [entries] + [_split(rng, e, 50) for e in ends if e > SMALL]
    ptr, ec, cnt, E = _n_of(cols)
    for frac in (0.5, 0.03):
        _agree(ptr, ec, cnt, E, [max(1, int(frac * c.sum())) for c in cols], seed=8)
    _agree(ptr, ec, cnt, E, [int(c.sum()) - 1 for c in cols], seed=8)


# ---- 4. the word boundary of the key ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,s,M,n", [SECOND_WORD[0], SECOND_WORD[2]], ids=["small", "large"])
def test_the_word_boundary_of_the_key(seed, s, M, n):
    o0, o1, o2, o3 = dc.key_words(seed, s, np.arange(M))
    order = np.lexsort((o0, o1, o2, o3))
    assert o3[order[n - 1]] == o3[order[n]]                                 # the n-th and the next read share the key's first word
    assert (M <= SMALL) == (M == SECOND_WORD[0][2])                          # one case for each path
    rng = np.random.default_rng(M)
    cols = [[] for _ in range(s)] + [_split(rng, M, 60)]
    target = np.full(s + 1, -1)
    for n_s in (n, n - 1, n + 1):                                           # the threshold between the two, and with either of them as the last
        target[s] = n_s
        _agree(*_n_of(cols), target, seed=seed)


# ---- 5. one rule for every route --------------------------------------------------------------------------------------------------------------
def _mixed():
    rng = np.random.default_rng(77)
    Ms = [1, 30, 700, SMALL, SMALL + 1, 9000, 3, 2 * WG + 1, 0, 12000]
    cols = [np.concatenate([_split(rng, M, int(rng.integers(1, 60))), np.zeros(int(rng.integers(0, 4)), dtype=np.int64)]) if M else np.zeros(2, dtype=np.int64)
            for M in Ms]
    return _n_of(cols) + (np.array(Ms),)


def _routes():
    ptr, ec, cnt, E, Ms = _mixed()
    half = Ms // 2
    want = dc.downsample(ptr, ec, cnt, E, half, 21)
    for tensors in (False, True, False):                                    # host entry, device entry, and a second call
        _agree(ptr, ec, cnt, E, half, seed=21, tensors=tensors, want=want)
    for s in range(len(Ms)):                                                # a sample's column whatever the other samples' targets are
        a, b = int(ptr[s]), int(ptr[s + 1])
        for others in (-1, 0):
            t = np.full(len(Ms), others)
            t[s] = half[s]
            got = _agree(ptr, ec, cnt, E, t, seed=21)[0]
            assert np.array_equal(got[a:b], want[0][a:b]), s
    assert not np.array_equal(dc.downsample(ptr, ec, cnt, E, half, 22)[0], want[0])      # (the seed counts)
    print("routes done")


def test_host_entry_device_entry_a_second_call_and_the_other_samples_targets():
    _routes()


def test_the_routes_and_the_shapes_with_the_scratch_poisoned():
    """One child process with ECB_POISON_SCRATCH=1: the pool is filled with 0x01 between calls, so a pass that relied on what scratch held
    gives another answer than the checker's."""
    env = dict(os.environ)
    env["ECB_POISON_SCRATCH"] = "1"
    env["ALNTOOLS_TORCH"] = "1"                     # (the child holds tensors: libecb and PyTorch share one HIP runtime, whatever this process set)
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_ecdownsample as t; t._routes(); "
            "[t.test_shapes_of_a_column(w) for w in t.SHAPES[:7]]; t.test_the_word_boundary_of_the_key(*t.SECOND_WORD[2]); print('poisoned cases done')"
            % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "poisoned cases done" in r.stdout


def test_nothing_to_thin():
    _agree([0], [], [], 5, [])                                              # no sample
    _agree([0, 0, 0], [], [], 5, [3, -1])                                   # no entry
    ptr, ec, cnt, E, Ms = _mixed()
    for t in (np.full(len(Ms), -1), Ms, Ms + 1):                            # every column copied: the call is a copy
        assert np.array_equal(_agree(ptr, ec, cnt, E, t)[0], cnt)
    assert not _agree(ptr, ec, cnt, E, np.zeros(len(Ms), dtype=np.int64))[0].any()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------
FILL = 0x5A5A5A5A


def _raw(ptr, ec, cnt, n_ecs, target, null=(), alias=None):
    """ecb_downsample itself on pre-filled outputs: (return code, message, whether every output is still as it was)."""
    lib = ed.load()
    a = [np.ascontiguousarray(x, dtype=np.int32) for x in (ptr, ec, cnt)] + [np.ascontiguousarray(target, dtype=np.int64)]
    S, nnz = len(a[0]) - 1, len(a[1])
    outs = [np.full(max(nnz, 1), FILL, dtype=np.int32), np.full(max(S, 1), FILL, dtype=np.int64), np.full(max(S, 1), FILL, dtype=np.int64)]
    p = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    ins = [None if k in null else p(x) for k, x in enumerate(a)]
    ous = [None if 4 + k in null else p(x) for k, x in enumerate(outs)]
    before = [x.copy() for x in a]
    if alias == "out_on_data":
        ous[0] = C.c_void_p(a[2].ctypes.data + 4)
    elif alias == "totals_on_target":
        ous[1] = ins[3]
    elif alias == "out_total_on_in_total":
        ous[2] = ous[1]
    rc = lib.ecb_downsample(0, n_ecs, S, nnz, ins[0], ins[1], ins[2], ins[3], 1, ous[0], ous[1], ous[2])
    same = all((o == FILL).all() for o in outs) and all(np.array_equal(x, y) for x, y in zip(a, before))
    return rc, (lib.ecb_last_error(None) or b"").decode(), same


def test_refusals_leave_every_output_untouched_and_the_next_call_works():
    ptr, ec, cnt, E, Ms = _mixed()
    half = Ms // 2
    mid = len(cnt) // 2

    def changed(x, at, v):
        y = np.array(x).copy()
        y[at] = v
        return y
    fall = changed(ptr, slice(3, 5), [ptr[4], ptr[3]])
    assert fall[4] < fall[3]
    for what, args, code, text in (
            ("a falling column pointer", (fall, ec, cnt, E, half), CONTRACT, "column pointers"),
            ("the first pointer", (changed(ptr, 0, 1), ec, cnt, E, half), CONTRACT, "column pointers"),
            ("the last pointer", (changed(ptr, -1, len(ec) - 1), ec, cnt, E, half), CONTRACT, "column pointers"),
            ("an EC index at n_ecs", (ptr, changed(ec, mid, E), cnt, E, half), CONTRACT, "an EC index at or beyond n_ecs"),
            ("a negative EC index", (ptr, changed(ec, 0, -1), cnt, E, half), CONTRACT, "an EC index at or beyond n_ecs"),
            ("a negative count", (ptr, ec, changed(cnt, len(cnt) - 1, -3), E, half), CONTRACT, "a negative count")):
        rc, msg, same = _raw(*args)
        assert rc == code and text in msg and same, (what, rc, msg)
        rc, msg, same = _raw(*args[:4], np.full(len(Ms), -1))                 # (malformed is malformed, whatever is asked for)
        assert rc == code and same, what
    # a sample of exactly 2^31 reads, as three entries: refused where it is thinned (n = 0 included), copied with n = -1
    top = (1 << 31) - 1
    big = ([0, 2, 5], [0, 1, 0, 1, 2], [4, 5, top, 1, 0], 3)
    for n in (0, 1, top):
        rc, msg, same = _raw(*big, [4, n])
        assert rc == LIMIT and "2^31 reads" in msg and same, (n, rc, msg)
    for n in (-1, 1 << 31, (1 << 31) + 5):
        out, tin, tout = ed.downsample(*big, [4, n])
        assert out.tolist() == dc.thin_column([4, 5], 0, 4, 0).tolist() + [top, 1, 0] and tin.tolist() == [9, 1 << 31] and tout.tolist() == [4, 1 << 31]
    for what, kw in (("no indptr_n", dict(null=(0,))), ("no indices_n", dict(null=(1,))), ("no data_n", dict(null=(2,))), ("no target", dict(null=(3,))),
                     ("no out_data_n", dict(null=(4,))), ("out_data_n over data_n", dict(alias="out_on_data")),
                     ("in_total on target", dict(alias="totals_on_target")), ("out_total on in_total", dict(alias="out_total_on_in_total"))):
        rc, msg, same = _raw(ptr, ec, cnt, E, half, **kw)
        assert rc == ARG and same, (what, rc, msg)
        assert "overlaps" in msg or "alias" not in kw, (what, msg)
    rc, msg, _ = _raw(ptr, ec, cnt, E, half, null=(5, 6))                    # the totals may be NULL
    assert rc == 0, msg
    _agree(ptr, ec, cnt, E, half, seed=1)                                   # the call after a refusal: the device is unharmed
