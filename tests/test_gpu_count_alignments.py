"""count-alignments on the GPU (``ecb_count_alignments`` / ``ecb_count_alignments_device``): the reference's arrays and table through the
Python function, the file command and the command line; the device entry against the host entry; random, boundary-sized, contended,
multisample and config-3-sized inputs against the numpy checker (``counts_checker.py``, itself equal to the reference on the goldens);
and every contract violation refused with the outputs untouched and the next call unharmed.

Sizes on the implementation's own limits (pinned in ``test_count_constants.py``): 1024 non-zeros per workgroup of the key pass, 16 384
per stretch of the prefix sum, CA_CHUNK = 32 768 sorted non-zeros per workgroup of the adding pass, the loci of one LDS window (2048 at
1 - 2 haplotypes, 512 at 8, 128 at 31) and 256 windows per pass of the sort."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from alntools_amd import bin_utils, ecb, methods

import counts_checker
import gt_checker

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CONTRACT = -5


def _cases(golden_dir):
    return [c for c in json.load(open(os.path.join(golden_dir, "counts_cases.json")))["cases"] if c["aln"] is not None]


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _same(got, exp, what=""):
    assert len(got) == len(exp) == 3
    for name, g, e in zip(("aln", "uniq", "locus_uniq"), got, exp):
        g = _np(g)
        assert g.dtype == np.int64 and g.shape == np.asarray(e).shape, (what, name)
        assert np.array_equal(g, e), (what, name, int((g != e).sum()))


def _one_sample(rng, n_ecs, absent=0.1, top=50):
    """N of a single-sample file: most ECs once, a share absent, some with count 0."""
    ecs = np.flatnonzero(rng.random(n_ecs) >= absent).astype(np.int32)
    return np.array([0, len(ecs)], dtype=np.int32), ecs, rng.integers(0, top, size=len(ecs)).astype(np.int32)


def _short_rows(rng, lens, n_loci, n_haps):
    """CSR with the given row lengths (each at most 8 and at most n_loci), columns strictly ascending, masks 1 .. 2^H - 1."""
    lens = np.asarray(lens, dtype=np.int64)
    assert lens.max(initial=0) <= min(8, n_loci)
    ip = np.concatenate([[0], np.cumsum(lens)])
    row = np.repeat(np.arange(len(lens)), lens)
    k = np.arange(int(ip[-1])) - ip[row]                              # place within the row
    g = max(1, n_loci // 8 - 1)
    gap = rng.integers(1, g + 1, size=int(ip[-1]))
    gap[k == 0] = 0
    c = np.cumsum(gap)
    c -= c[ip[row]]                                                   # offset from the row's first column
    span = np.zeros(len(lens), dtype=np.int64)
    np.maximum.at(span, row, c)
    start = (rng.random(len(lens)) * (n_loci - span)).astype(np.int64)
    col = start[row] + c
    assert col.max(initial=0) < n_loci
    da = rng.integers(1, 1 << n_haps, size=int(ip[-1]), dtype=np.int64)
    return ip.astype(np.int32), col.astype(np.int32), da.astype(np.int32)


def _check(ip, ix, da, T, H, N, sample=None, what=""):
    got = ecb.count_alignments(ip, ix, da, T, H, *N, sample=sample)
    _same(got, counts_checker.count(ip, ix, da, T, H, *N, sample=sample), what)
    return got


# ---- the reference's numbers, through three routes ---------------------------------------------------------------------------------------

def test_goldens_through_ecb_count_alignments(golden_dir):
    for c in _cases(golden_dir):
        m = bin_utils.ecload(os.path.join(golden_dir, c["bin"]))
        got = ecb.count_alignments(m.indptrA, m.indicesA, m.dataA, m.num_loci, m.num_haplotypes, m.indptrN, m.indicesN, m.dataN)
        _same(got, counts_checker.golden_arrays(c), c["bin"])


def _golden_text(golden_dir, c):
    m = bin_utils.ecload(os.path.join(golden_dir, c["bin"]))
    aln, uniq, lu = (a.astype(np.float64) for a in counts_checker.golden_arrays(c))     # (the reference's sums are float64)
    cnt = np.vstack((aln, uniq, lu))
    text = "locus\t" + "\t".join("aln_%s" % h for h in m.hname) + "\t" + "\t".join("uniq_%s" % h for h in m.hname) + "\tlocus_uniq\n"
    for t in range(m.num_loci):
        text += "\t".join([m.lname[t]] + list(map(str, cnt[:, t].ravel()))) + "\n"        # AlignmentPropertyMatrix.py:461
    return text


def test_goldens_through_methods_count_alignments(golden_dir, tmp_path):
    for c in _cases(golden_dir):
        out = str(tmp_path / (c["bin"] + ".tsv"))
        methods.count_alignments(os.path.join(golden_dir, c["bin"]), out)
        assert open(out).read() == _golden_text(golden_dir, c), c["bin"]


def test_goldens_through_the_command_line_import_no_pytorch(golden_dir, tmp_path):
    env = dict(os.environ)
    env.pop("ALNTOOLS_TORCH", None)
    env.pop("ALNTOOLS_GPUS", None)
    for c in _cases(golden_dir):
        if c["bin"] not in ("g1_edge.bin", "gt_h8_in.bin"):
            continue
        out = str(tmp_path / (c["bin"] + ".tsv"))
        r = subprocess.run([sys.executable, "-X", "importtime", "-m", "alntools_amd.cli", "count-alignments", os.path.join(golden_dir, c["bin"]),
                            out, "-v"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        imported = [l.split("|")[-1].strip() for l in r.stderr.splitlines() if l.startswith("import time:")]
        assert "alntools_amd.ecb" in imported
        assert not any(m == "torch" or m.startswith("torch.") for m in imported)
        assert "Error:" not in r.stderr, r.stderr[-2000:]
        assert open(out).read() == _golden_text(golden_dir, c), c["bin"]


def test_unknown_sample_is_logged_and_exits_1(golden_dir, tmp_path):
    out = str(tmp_path / "none.tsv")
    r = subprocess.run([sys.executable, "-m", "alntools_amd.cli", "count-alignments", os.path.join(golden_dir, "g4_multi_min0.bin"), out,
                        "-s", "no_such_sample"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "Error: " in r.stderr and "no_such_sample" in r.stderr
    assert not os.path.exists(out)


def test_multisample_file_all_samples_and_one_named(golden_dir, tmp_path):
    path = os.path.join(golden_dir, "g4_multi_min0.bin")
    m = bin_utils.ecload(path)
    for s, name in [(None, None), (m.num_samples - 1, m.sname[-1])]:
        out = str(tmp_path / "ms.tsv")
        bin_utils.count_alignments(path, out, sample=name)
        exp = counts_checker.count(m.indptrA, m.indicesA, m.dataA, m.num_loci, m.num_haplotypes, m.indptrN, m.indicesN, m.dataN, sample=s)
        assert open(out).read() == bin_utils.counts_table(m.lname, m.hname, *exp)


def test_device_entry_equals_host_entry(golden_dir):
    import torch
    m = bin_utils.ecload(os.path.join(golden_dir, "gt_h8_in.bin"))
    arrays = (m.indptrA, m.indicesA, m.dataA, m.indptrN, m.indicesN, m.dataN)
    host = ecb.count_alignments(*arrays[:3], m.num_loci, m.num_haplotypes, *arrays[3:])
    d = [torch.from_numpy(a.astype(np.int32)).cuda() for a in arrays]
    dev = ecb.count_alignments(*d[:3], m.num_loci, m.num_haplotypes, *d[3:])
    assert all(t.is_cuda and t.dtype == torch.int64 for t in dev)
    _same(dev, host)
    _same(host, counts_checker.count(*arrays[:3], m.num_loci, m.num_haplotypes, *arrays[3:]))


# ---- shapes ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_haps", [1, 2, 8, 31])
def test_random_csrs_against_the_checker(n_haps):
    rng = np.random.default_rng(300 + n_haps)
    for n_ecs, n_loci in ((1, 1), (1, 900), (7, 3), (4097, 1000), (70_001, 5_000)):
        ip, ix, da = gt_checker.random_csr(rng, n_ecs, n_loci, n_haps)
        _check(ip, ix, da, n_loci, n_haps, _one_sample(rng, n_ecs), what=(n_ecs, n_loci))


def test_fixed_small_cases():
    rng = np.random.default_rng(11)
    N = lambda E: (np.array([0, E], np.int32), np.arange(E, dtype=np.int32), np.arange(1, E + 1, dtype=np.int32))   # noqa: E731
    none = np.zeros(0, np.int32)
    # empty rows only, which is also nnz_a = 0
    got = _check(np.zeros(6, np.int32), none, none, 4, 2, N(5), what="empty rows")
    assert not any(_np(g).any() for g in got)
    _check(np.zeros(1, np.int32), none, none, 1, 1, (np.zeros(2, np.int32), none, none), what="no ECs at all")
    # nnz_n = 0: everything is 0
    ip, ix, da = gt_checker.random_csr(rng, 500, 300, 4)
    got = _check(ip, ix, da, 300, 4, (np.zeros(2, np.int32), none, none), what="nnz_n = 0")
    assert not any(_np(g).any() for g in got)
    # zero masks: no non-zero, no bit -- rows that are unique only because their other entries are 0, and rows of zeros alone
    z = da.copy()
    z[rng.random(len(z)) < 0.6] = 0
    _check(ip, ix, z, 300, 4, N(500), what="zero masks")
    _check(ip, ix, np.zeros_like(da), 300, 4, N(500), what="all masks zero")
    ip2 = np.array([0, 3, 5, 6], np.int32)
    got = _check(ip2, np.array([1, 2, 5, 0, 5, 3], np.int32), np.array([0, 2, 0, 3, 0, 0], np.int32), 6, 2, N(3), what="hand-made zeros")
    assert _np(got[1])[1, 2] == 1 and _np(got[2])[2] == 1 and _np(got[2])[0] == 2 and _np(got[1]).sum() == 1
    # rows of 64, 65, 1024 and 1025 non-zeros, between rows of one
    lens = [1, 64, 1, 65, 1024, 1, 1, 1025, 1]
    T = 1500
    ip = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ix = np.concatenate([np.sort(rng.choice(T, size=k, replace=False)) for k in lens]).astype(np.int32)
    da = rng.integers(1, 256, size=len(ix)).astype(np.int32)
    _check(ip, ix, da, T, 8, N(len(lens)), what="rows of 64 .. 1025")


@pytest.mark.parametrize("nnz", [1023, 1024, 1025, 16383, 16384, 16385, 32767, 32768, 32769, 65537])
def test_non_zeros_on_the_workgroup_limits(nnz):
    """1024 per workgroup of the key pass, 16 384 per stretch of the prefix sum, 32 768 per workgroup of the adding pass."""
    rng = np.random.default_rng(nnz)
    lens = rng.integers(0, 5, size=nnz)                               # rows of 0 - 4, cut to the wanted number of non-zeros
    lens = lens[:int(np.searchsorted(np.cumsum(lens), nnz, side="right"))]
    lens = np.append(lens, nnz - lens.sum())
    assert lens.sum() == nnz and lens.max() <= 8
    ip, ix, da = _short_rows(rng, lens, 3000, 8)
    _check(ip, ix, da, 3000, 8, _one_sample(rng, len(lens)), what=nnz)


@pytest.mark.parametrize("n_haps,window", [(1, 2048), (2, 2048), (8, 512), (31, 128)])
def test_loci_on_the_window_and_sort_pass_limits(n_haps, window):
    """One window less one, exactly one, one and a locus; 256 windows (one digit of the sort) less one locus, exactly, and one more."""
    rng = np.random.default_rng(n_haps)
    for T in (window - 1, window, window + 1, 256 * window - 1, 256 * window, 256 * window + 1):
        lens = rng.integers(0, 5, size=3000)
        ip, ix, da = _short_rows(rng, lens, T, n_haps)
        ix[:: 7] = np.where(np.diff(ip)[np.searchsorted(ip, np.arange(0, len(ix), 7), side="right") - 1] == 1, T - 1, ix[:: 7])  # lone entries: the last locus
        _check(ip, ix, da, T, n_haps, _one_sample(rng, 3000), what=T)


# ---- contention and width ----------------------------------------------------------------------------------------------------------------

def test_one_counter_takes_every_add_past_32_bits():
    E, w = 200_000, 2 ** 31 - 1
    N = (np.array([0, E], np.int32), np.arange(E, dtype=np.int32), np.full(E, w, dtype=np.int32))
    ip = np.arange(E + 1, dtype=np.int32)
    aln, uniq, lu = (_np(a) for a in ecb.count_alignments(ip, np.zeros(E, np.int32), np.ones(E, np.int32), 700, 3, *N))
    assert E * w > 2 ** 32
    assert aln[0, 0] == uniq[0, 0] == lu[0] == E * w
    assert aln.sum() == uniq.sum() == lu.sum() == E * w
    # every row also holds a second locus: nothing is unique
    ip = (2 * np.arange(E + 1)).astype(np.int32)
    ix = np.zeros(2 * E, np.int32)
    ix[1::2] = 1 + np.arange(E) % 699
    aln, uniq, lu = (_np(a) for a in ecb.count_alignments(ip, ix, np.ones(2 * E, np.int32), 700, 3, *N))
    assert aln[0, 0] == E * w and aln.sum() == 2 * E * w and not uniq.any() and not lu.any()


def test_multisample_weights():
    rng = np.random.default_rng(21)
    E, T, H = 5000, 800, 4
    ip, ix, da = gt_checker.random_csr(rng, E, T, H)
    cols = [np.sort(rng.choice(E, size=k, replace=False)) for k in (3000, 0, 1200)]
    cols[2] = np.sort(np.concatenate([cols[2], cols[2][:40], [cols[2][0]]]))        # ECs listed twice, one three times
    N = (np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32), np.concatenate(cols).astype(np.int32),
         rng.integers(0, 1000, size=sum(len(c) for c in cols)).astype(np.int32))
    for s in (None, 0, 1, 2):
        _check(ip, ix, da, T, H, N, sample=s, what=s)
    w = counts_checker.weights(E, *N, sample=2)
    assert w[cols[2][0]] == N[2][N[0][2]:][cols[2] == cols[2][0]].sum()          # (the checker adds duplicates too)


# ---- the contract ------------------------------------------------------------------------------------------------------------------------

def test_contract_violations_leave_the_outputs_untouched_and_the_next_call_works():
    import torch
    lib = ecb.load()
    rng = np.random.default_rng(5)
    E, T, H = 3000, 500, 4
    ip, ix, da = gt_checker.random_csr(rng, E, T, H)
    pn = np.array([0, 1000, 1000, 2500], dtype=np.int32)
    xn = np.concatenate([np.sort(rng.choice(E, size=k, replace=False)) for k in (1000, 0, 1500)]).astype(np.int32)
    dn = rng.integers(0, 90, size=2500).astype(np.int32)
    good = counts_checker.count(ip, ix, da, T, H, pn, xn, dn)
    a = int(ip[int(np.argmax(np.diff(ip)))])
    ok = dict(ip=ip, ix=ix, da=da, pn=pn, xn=xn, dn=dn, sample=-1)
    bad = []

    def breach(what, **kw):
        bad.append((what, dict(ok, **kw)))

    p = ip.copy(); p[0] = 1; breach("indptr[0] != 0", ip=p)
    p = ip.copy(); p[-1] -= 1; breach("indptr[E] != nnz", ip=p)
    p = ip.copy(); p[10], p[11] = p[11] + 1, p[10]; breach("falling indptr", ip=p)
    p = ip.copy(); p[20] = len(ix) + 5; breach("indptr beyond nnz", ip=p)
    x = ix.copy(); x[5] = T; breach("locus >= T", ix=x)
    x = ix.copy(); x[7] = -1; breach("negative locus", ix=x)
    x = ix.copy(); x[a + 1], x[a + 2] = x[a + 2], x[a + 1]; breach("unsorted column", ix=x)
    x = ix.copy(); x[a + 2] = x[a + 1]; breach("duplicate column", ix=x)
    d = da.copy(); d[9] = 1 << H; breach("bit >= H", da=d)
    p = pn.copy(); p[0] = 1; breach("N pointers not from 0", pn=p)
    p = pn.copy(); p[-1] = 2499; breach("N pointers not to nnz_n", pn=p)
    p = pn.copy(); p[1], p[2] = 1200, 1100; breach("N pointers falling", pn=p)
    x = xn.copy(); x[3] = E; breach("EC >= n_ecs", xn=x)
    x = xn.copy(); x[4] = -2; breach("negative EC", xn=x)
    d = dn.copy(); d[2400] = -1; breach("negative count", dn=d)
    breach("sample = n_samples", sample=3)
    breach("sample = -2", sample=-2)

    def call(k, host):
        arrs = [np.ascontiguousarray(k[n], dtype=np.int32) for n in ("ip", "ix", "da", "pn", "xn", "dn")]
        if host:
            outs = [np.full((H, T), 7, np.int64), np.full((H, T), 7, np.int64), np.full(T, 7, np.int64)]
            ptr = lambda v: v.ctypes.data_as(C.c_void_p)   # noqa: E731
            fn = lib.ecb_count_alignments
        else:
            arrs = [torch.from_numpy(v).cuda() for v in arrs]
            outs = [torch.full((H, T), 7, dtype=torch.int64, device="cuda"), torch.full((H, T), 7, dtype=torch.int64, device="cuda"),
                    torch.full((T,), 7, dtype=torch.int64, device="cuda")]
            ptr = lambda v: C.c_void_p(v.data_ptr())       # noqa: E731
            fn = lib.ecb_count_alignments_device
        rc = fn(0, E, T, H, len(ix), ptr(arrs[0]), ptr(arrs[1]), ptr(arrs[2]), 3, len(xn), ptr(arrs[3]), ptr(arrs[4]), ptr(arrs[5]), k["sample"],
                ptr(outs[0]), ptr(outs[1]), ptr(outs[2]))
        return rc, [_np(o) for o in outs]

    for host in (False, True):
        for what, k in bad:
            rc, outs = call(k, host)
            assert rc == CONTRACT, (what, host, rc, lib.ecb_last_error(None))
            assert all((o == 7).all() for o in outs), (what, host)
            rc, outs = call(ok, host)                                  # the device is unharmed
            assert rc == 0, (what, host)
            _same(outs, good, what)


def test_null_outputs_are_skipped():
    lib = ecb.load()
    rng = np.random.default_rng(9)
    ip, ix, da = gt_checker.random_csr(rng, 200, 100, 3)
    N = _one_sample(rng, 200)
    exp = counts_checker.count(ip, ix, da, 100, 3, *N)
    lu = np.full(100, 7, np.int64)
    ptr = lambda v: v.ctypes.data_as(C.c_void_p)   # noqa: E731
    rc = lib.ecb_count_alignments(0, 200, 100, 3, len(ix), ptr(ip), ptr(ix), ptr(da), 1, len(N[1]), ptr(N[0]), ptr(N[1]), ptr(N[2]), -1, None, None, ptr(lu))
    assert rc == 0 and np.array_equal(lu, exp[2])


# ---- config 3 ----------------------------------------------------------------------------------------------------------------------------

def test_config3_sized_matrix_against_the_checker():
    ip, ix, da, T, H = gt_checker.c3_csr()
    E = len(ip) - 1
    rng = np.random.default_rng(4)
    N = (np.array([0, E], dtype=np.int32), np.arange(E, dtype=np.int32), rng.integers(1, 100, size=E).astype(np.int32))
    _check(ip, ix, da, T, H, N, what="config 3")
