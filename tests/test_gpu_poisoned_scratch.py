"""Every entry point of libecb with its scratch memory poisoned (``ECB_POISON_SCRATCH``: every device allocation of the library filled
with 0x01 before it is handed out, dead pool buffers filled again at ``ecb_reset`` and at the end of a handle-less call -- DESIGN.md
section 4).  A kernel that reads scratch nobody wrote -- a forgotten memset, one that covers n words of n + 1 -- sees zeros after a fresh
hipMalloc and the right answer of the test before in a pool buffer; under the switch it sees 0x01010101.

Every case runs twice: with the switch off (the case itself is right), then on (the test).  Results are compared bit for bit with the
authorities the rest of the suite trusts: the C oracle, the numpy checkers, scipy.  The shapes are the smallest that reach the path
named; the generators are the other GPU tests' own."""
import ctypes as C

import numpy as np
import pytest

from alntools_amd import bin_utils, ecb
from oracle import c_oracle
from oracle import ec_oracle as orc

import counts_checker
import ec_merge_checker as chk
import gt_checker
import salmon_checker as schk
import test_gpu_count_alignments as tca
import test_gpu_ecbundle as tb
import test_gpu_ecmerge as tmg
import test_gpu_multisample as tm
import test_gpu_thresholds as th
from test_bundle_constants import FOLD_TPB, WAVE
from test_gpu_parity import _check

pytestmark = pytest.mark.gpu

CONTRACT = -5
SMALL = dict(ec_capacity=1 << 12, arena_capacity=1 << 24)       # (4 096 slots, 128 MB of key arena: nothing of 1 GB is filled per handle)


@pytest.fixture(params=["off", "on"])
def poison(request, monkeypatch):
    """The switch through the case's parameter: off first, then on."""
    if request.param == "on":
        monkeypatch.setenv("ECB_POISON_SCRATCH", "1")
    else:
        monkeypatch.delenv("ECB_POISON_SCRATCH", raising=False)
    return request.param == "on"


# ---- the stream path and finalize -------------------------------------------------------------------------------------------------------
def _reads(rng, n, T, H, longest=12):
    """n reads of 1 .. ``longest`` records on distinct loci."""
    return [th._distinct(rng, int(rng.integers(1, longest + 1)), T, H) for _ in range(n)]


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _short_stream():
    def make():
        rng = np.random.default_rng(41)
        T, H = 2000, 8
        t = th._stream(_reads(rng, 3000, T, H))
        return t, T, H, th._oracle(t, H)
    return _cached("short", make)


def _finished(b, exp, dev=None):
    """finalize, export, export_read_ec and (after a device push) the exactness pass of a handle that holds the stream of ``exp``."""
    s = b.finalize()
    _check(b.export(), s, exp)
    ec = b.export_read_ec()
    assert len(ec) == s["n_reads"] and np.array_equal(np.bincount(ec, minlength=s["n_ecs"]), exp["count"])
    if dev is not None:
        assert b.verify_device(*dev)[0] == 0


@pytest.mark.parametrize("compilation", sorted(th.COMPILATIONS))
def test_every_push_through_every_compilation(poison, compilation, monkeypatch):
    """3 000 reads of up to 12 records through ecb_push (one batch, batches of 777), ecb_push_device and ecb_push_device_tiled, each of
    the stream kernel's compilations forced in turn; finalize, export, export_read_ec, verify_device = 0."""
    t, T, H, exp = _short_stream()
    env, hinted, kernel = th.COMPILATIONS[compilation]
    th._force(monkeypatch, env)
    d = th._dev(t)
    n = len(t["read_id"])
    for how in ("host", "host777", "device", "tiled"):
        with ecb.EcBuilder(T, H, **SMALL) as b:
            if hinted:
                b.hint_reads(exp["n_reads"])
            if how == "device":
                b.push_device(*d)
            elif how == "tiled":
                b.push_device_tiled(ecb.tile_tuples(*d), n)
            else:
                step = 777 if how == "host777" else n
                for a in range(0, n, step):
                    b.push(*(t[k][a:a + step] for k in ("read_id", "locus", "hapflag")))
                b.counters()                                             # (the carried read goes in: the kernel's name is the last batch's)
            assert b.profile_kernel().startswith(kernel), (how, b.profile_kernel())
            _finished(b, exp, d)


def test_table_that_grows_and_ecs_past_one_scan_stretch(poison):
    """``ec_capacity=64`` gives the smallest table the library makes (``ecb_create``: 1 024 slots); it is kept at most half full and grows
    four-fold (``process_batch``), so holding more than 16 384 ECs -- one stretch of the scan -- takes three growths while batches arrive
    (k_rehash, k_remap_read_slot of the reads before).  Rows on both sides of the five inline pairs, and keys that go one wave each through
    the emit (17, 2 049 and 5 003 pairs)."""
    def make():
        rng = np.random.default_rng(42)
        T, H = 30_000, 8
        reads = _reads(rng, 9000, T, H) + th._key_reads(rng, T, H, (17, 2049, 5003)) + _reads(rng, 9000, T, H)
        t = th._stream(reads)
        return t, T, H, th._oracle(t, H)
    t, T, H, exp = _cached("grow", make)
    assert len(exp["count"]) > 16_384 and (np.diff(exp["indptr"]) <= 5).any() and (np.diff(exp["indptr"]) > 2048).any()
    d = th._dev(t)
    cuts = np.searchsorted(t["read_id"], np.arange(0, exp["n_reads"] + 2999, 3000))
    with ecb.EcBuilder(T, H, ec_capacity=64, arena_capacity=1 << 24) as b:
        for a, z in zip(cuts[:-1], cuts[1:]):
            if a % 4 == 0:                                               # (a device stream starts on 16 bytes)
                b.push_device(*(x[a:z] for x in d))
            else:
                b.push(*(t[k][a:z] for k in ("read_id", "locus", "hapflag")))
                b.counters()                                             # (the read the host push left open goes in)
        assert b.table_sizes()[0] == len(exp["count"]) > 16 * 1024       # (entries held: more than 1 024 x 4 x 4 slots could, half full)
        _finished(b, exp, d)


def test_reads_for_k_slow_in_lds_and_in_global_scratch(poison):
    """Reads of 81 to 300 distinct entries (k_slow, its table in LDS) and one of more than 2 048 records (its table in global scratch,
    which k_slow must leave zeroed for the next round), between short reads; twice on one handle."""
    def make():
        rng = np.random.default_rng(43)
        T, H = 20_000, 8
        reads = []
        for L in (81, 300, 2500, 150, 299):
            reads += th._fill(rng, int(rng.integers(200, 700)), T, H) + [th._distinct(rng, L, T, H)]
        reads += th._fill(rng, 1500, T, H)
        t = th._stream(reads)
        return t, T, H, th._oracle(t, H)
    t, T, H, exp = _cached("slow", make)
    d = th._dev(t)
    with ecb.EcBuilder(T, H, **SMALL) as b:
        b.push_device(*d)
        _finished(b, exp, d)
        b.reset()
        b.push(t["read_id"], t["locus"], t["hapflag"])
        _finished(b, exp)


def test_ranges_against_numpy_min_max(poison):
    """``track_ranges``: export_ranges and export_range_minmax == numpy's per-(locus, haplotype) min / max over the valid records."""
    import torch
    rng = np.random.default_rng(44)
    T, H = 1500, 4
    reads = []
    for _ in range(1200):
        loci, haps = th._distinct(rng, int(rng.integers(1, 12)), T, H)
        flags = np.where(rng.random(len(loci)) < 0.1, 0x4, 0).astype(np.uint32)
        flags[0] = 0
        reads.append((loci, haps, flags))
    t = th._stream(reads)
    n = len(t["read_id"])
    pos = rng.integers(0, (1 << 31) - 1, size=n).astype(np.int64)
    t["pos"] = pos.astype(np.int32)
    valid = orc.tuples_valid(t["hapflag"])
    slot = t["locus"].astype(np.int64) * H + ((t["hapflag"].astype(np.int64) >> 16) & 0xFF)
    mn = np.full(T * H, np.iinfo(np.int32).max, np.int64)
    mx = np.full(T * H, np.iinfo(np.int32).min, np.int64)
    np.minimum.at(mn, slot[valid], pos[valid])
    np.maximum.at(mx, slot[valid], pos[valid])
    length = np.where(mx == np.iinfo(np.int32).min, 0, mx - mn + 1)
    exp = th._oracle(t, H)
    d = th._dev(t) + [torch.from_numpy(t["pos"]).cuda()]
    for device in (False, True):
        with ecb.EcBuilder(T, H, track_ranges=True, **SMALL) as b:
            for k in range(2):                                           # (and again after a reset: the ranges start over)
                if device:
                    b.push_device(*d)
                else:
                    b.push(t["read_id"], t["locus"], t["hapflag"], t["pos"])
                _check(b.export(), b.finalize(), exp)
                assert np.array_equal(b.export_ranges().reshape(-1), length)
                gmn, gmx = b.export_range_minmax()
                assert np.array_equal(gmn.reshape(-1), mn) and np.array_equal(gmx.reshape(-1), mx)
                b.reset()


def test_one_handle_finalized_twice_then_reused_smaller_and_larger(poison):
    """A second finalize; reset and a stream of a tenth of the size (fewer reads, fewer ECs, shorter rows: every pool buffer reused dirty
    at a smaller size); reset and a larger stream (every pool buffer regrown)."""
    def make():
        rng = np.random.default_rng(45)
        T, H = 5000, 8
        out = []
        for n, longest in ((4000, 12), (400, 4), (9000, 40)):
            t = th._stream(_reads(rng, n, T, H, longest))
            out.append((t, th._oracle(t, H)))
        return T, H, out
    T, H, streams = _cached("reuse", make)
    with ecb.EcBuilder(T, H, **SMALL) as b:
        for k, (t, exp) in enumerate(streams):
            if k:
                b.reset()
            d = th._dev(t)
            if k == 1:
                b.push(t["read_id"], t["locus"], t["hapflag"])
            else:
                b.push_device(*d)
            _finished(b, exp)
            _finished(b, exp, d)                                         # (the second finalize, and the exactness pass behind it)


# ---- multisample ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("n_cells", [100, 8193])
def test_multisample_filter_on_both_paths_of_the_cell_totals(poison, n_cells, device):
    """push_cells from the host and from the device, export_pairs, ms_filter + ms_export at 100 cells (k_msf2_cells adds in LDS) and 8 193
    (in memory), minimum counts 0 and one that removes cells and ECs, the same handle filtered twice."""
    def make():
        st = tm._random_stream(np.random.default_rng(46 + n_cells), np.arange(n_cells), 3 * n_cells + 3000, 3, n_tpl=600)
        return st, st.expected()
    st, exp = _cached(("ms", n_cells), make)
    tr, n_ecs = exp[0], exp[1]
    totals = np.bincount(tr["cell"], weights=tr["count"], minlength=n_cells)
    cut = int(np.quantile(totals, 0.6)) + 1
    with ecb.EcBuilder(st.n_loci, tm.H, multisample=True, **SMALL) as b:
        tm._push(b, st, device)
        a = tm._check_built(b, st, exp)
        for mc in (0, cut, 0, cut):
            kept = tm._check_filter(b, a, tr, n_ecs, n_cells, mc)
            assert (len(kept) == n_cells) == (mc == 0)
        assert b.ms_filter_sizes(n_cells, cut)["n_ecs_kept"] < n_ecs


# ---- several shards on one card ---------------------------------------------------------------------------------------------------------
def _shard_stream():
    def make():
        rng = np.random.default_rng(47)
        T, H = 8000, 8
        reads = _reads(rng, 1500, T, H) + th._key_reads(rng, T, H, (6, 17, 2049)) + _reads(rng, 1500, T, H)
        reads += [reads[k] for k in rng.integers(0, len(reads), 1500)]      # (ECs that the shards share)
        t = th._stream(reads)
        return t, T, H, th._oracle(t, H), len(reads)
    return _cached("shards", make)


def _shards(t, T, H, cut_reads):
    cuts = [int(np.searchsorted(t["read_id"], r)) for r in cut_reads]
    out = []
    for a, z in zip(cuts[:-1], cuts[1:]):
        b = ecb.EcBuilder(T, H, ec_capacity=1 << 10, arena_capacity=1 << 24)
        b.push(t["read_id"][a:z] - t["read_id"][a], t["locus"][a:z], t["hapflag"][a:z])
        out.append(b)
    return out


@pytest.mark.parametrize("n_shards", [2, 3])
def test_shards_merged_by_key_range_adopted_assembled_and_merged_inside_the_library(poison, n_shards):
    """Shards cut at read boundaries: table_export_parts -> table_merge_batch -> table_adopt_batch -> finalize; table_rebase -> merge ->
    finalize per range -> assemble_ranges; ecb_merge -- each == the C oracle over the whole stream."""
    import torch
    from alntools_amd import dist as ecdist
    dev = torch.device("cuda:0")
    t, T, H, exp, R = _shard_stream()
    cut_reads = [0, R // 3, R] if n_shards == 2 else [0, R // 4, R // 2 + 7, R]
    P = n_shards
    mk = lambda: ecdist.GpuEngine(ecb.EcBuilder(T, H, ec_capacity=1 << 10, arena_capacity=1 << 24), dev)   # noqa: E731
    # by key range, adopted
    pieces, counts, base = [], [], 0
    for b in _shards(t, T, H, cut_reads):
        nreads = b.table_sizes()[2]
        pieces.append(ecdist.GpuEngine(b, dev).table_export_parts(base, P))
        counts.append(b.counters()[:2])
        base += nreads
        b.close()
    root, adopted = mk(), []
    for q in range(P):
        part = mk()
        part.table_merge_many([(ent[eo[q] * 4:eo[q + 1] * 4], eo[q + 1] - eo[q], prs[po[q]:po[q + 1]], po[q + 1] - po[q])
                               for ent, prs, eo, po in pieces if eo[q + 1] > eo[q]])
        pe_n, pp_n, _ = part.table_sizes()
        adopted.append(part.table_export(0) + (pe_n, pp_n))
        part.b.close()
    root.table_adopt_many([(pe, pe_n, pp, pp_n) for pe, pp, pe_n, pp_n in adopted])
    root.add_counters(sum(c[0] for c in counts), sum(c[1] for c in counts), base)
    _check(root.b.export(), root.b.finalize(), exp)
    root.b.close()
    # every range finalized on its own handle, the pieces assembled
    cuts, bases, base, totals, shards = [], [], 0, [0, 0, 0], _shards(t, T, H, cut_reads)
    for b in shards:
        eng = ecdist.GpuEngine(b, dev)
        cuts.append(eng.table_export_parts(0, P))
        bases.append(base)
        a, v, n = eng.counters()
        totals = [totals[0] + a, totals[1] + v, totals[2] + n]
        base += n
    ranges = []
    for q in range(P):
        part = mk()
        part.table_merge_many([(part.table_rebase(ent[eo[q] * 4:eo[q + 1] * 4], eo[q + 1] - eo[q], rb), eo[q + 1] - eo[q], prs[po[q]:], po[q + 1] - po[q])
                               for (ent, prs, eo, po), rb in zip(cuts, bases) if eo[q + 1] > eo[q]])
        ranges.append(part.finalize_range(*totals))
        part.b.close()
    for b in shards:
        b.close()
    root = mk()
    s = root.assemble_ranges([p for p in ranges if p[1]], *totals)
    _check(root.b.export(), s, exp)
    root.b.close()
    # inside the library
    sh = _shards(t, T, H, cut_reads)
    with ecb.EcBuilder(T, H, ec_capacity=1 << 10, arena_capacity=1 << 24) as r2:
        s = r2.merge_from(sh)
        _check(r2.export(), s, exp)
    for b in sh:
        b.close()


@pytest.mark.parametrize("n_shards", [2, 3])
def test_multisample_triples_over_shards_equal_one_handle(poison, n_shards):
    """ms_local_triples on every shard, ms_adopt_triples on the root == the triples of one handle (the stream's own expectation)."""
    def make():
        st = tm._random_stream(np.random.default_rng(48), np.arange(300) * 5, 6000, 4, n_tpl=500)
        return st, st.expected()
    st, exp = _cached("ms_shards", make)
    tr, n_ecs = exp[0], exp[1]
    cuts = [0, 2501, st.n_reads] if n_shards == 2 else [0, 1999, 4000, st.n_reads]
    root, shards = tm._sharded(st, cuts)
    try:
        got = root.b.export_pairs()
        for k in ("ec", "cell", "file", "count", "first"):
            assert np.array_equal(got[k], tr[k]), k
        a = root.b.export()
        for k, e in zip(("indptrA", "indicesA", "dataA"), exp[2]):
            assert np.array_equal(a[k], e), k
        tm._check_filter(root.b, a, tr, n_ecs, 1500, 3)
    finally:
        root.b.close()
        for b in shards:
            b.close()


# ---- the entry points that take no handle ---------------------------------------------------------------------------------------------------
def _hapcsc(E, T, H, r, c, b):
    """(row, column, haplotype) triples -> (CSR with bitmask values, per-haplotype CSC), both by scipy."""
    from scipy import sparse
    ref = sparse.coo_matrix(((1 << b).astype(np.int64), (r, c)), shape=(E, T)).tocsr()
    ref.sort_indices()
    cps, cis = [], []
    for h in range(H):
        sel = b == h
        mh = sparse.coo_matrix((np.ones(int(sel.sum()), np.int8), (r[sel], c[sel])), shape=(E, T)).tocsc()
        mh.sort_indices()
        cps.append(mh.indptr.astype(np.int32)); cis.append(mh.indices.astype(np.int32))
    csr = tuple(np.ascontiguousarray(x, dtype=np.int32) for x in (ref.indptr, ref.indices, ref.data))
    return csr, (np.stack(cps), np.concatenate(cis))


def _conversion_case(name):
    """E, T, H and the matrix as (row, column, haplotype): one long column (spread over all ECs: cut into pieces and hashed; bunched: 4 000
    row indices within 5 000 ECs, entry by entry), an empty haplotype, empty columns; more than 4 096 non-zeros in all."""
    rng = np.random.default_rng({"spread": 6, "bunched": 7, "shuffled": 7, "h31": 3}[name])   # (shuffled: the matrix of bunched)
    E, T, H = (20_000, 12, 3) if name != "h31" else (3000, 40, 31)
    r, c, b = [], [], []

    def column(col, per_hap, span):
        for h, k in enumerate(per_hap):
            r.append(rng.choice(span, size=k, replace=False)); c.append(np.full(k, col)); b.append(np.full(k, h))
    if name == "spread":
        column(0, (1200, 0, 2100), E)                                    # 3 300 > 3 072, haplotype 1 empty in it
    elif name in ("bunched", "shuffled"):
        column(0, (2000, 0, 2000), 5000)
    for col in range(2, T, 2):                                           # (odd columns stay empty; haplotype 1 holds nothing at all)
        column(col, [int(rng.integers(0, 400)) if h != 1 else 0 for h in range(H)], E)
    r, c, b = np.concatenate(r), np.concatenate(c), np.concatenate(b)
    return E, T, H, r, c, b


@pytest.mark.parametrize("name", ["spread", "bunched", "shuffled", "h31"])
def test_conversions_between_csr_and_per_haplotype_csc(poison, name):
    """csr_to_hapcsc and hapcsc_to_csr, device and host entries, against scipy.  ``shuffled``: the long column's lists in random order --
    the sort-everything path, in buffers of its own."""
    import torch
    E, T, H, r, c, b = _conversion_case(name)
    csr, (cp, ci) = _cached(("conv", name), lambda: _hapcsc(E, T, H, r, c, b))
    assert len(csr[1]) > 4096 and (name == "h31" or not (b == 1).any())
    ci_in = ci.copy()
    if name == "shuffled":
        rng = np.random.default_rng(3)
        starts = np.concatenate(([0], np.cumsum(cp[:, -1])))
        for h in range(H):
            a, z = starts[h] + cp[h, 0], starts[h] + cp[h, 1]
            ci_in[a:z] = rng.permutation(ci_in[a:z])
        # (what sends the call down that path, ``ecb.hip: CVB_ERR_ORDER``: a column of more than CVU_MAX = 3 072 row indices with a list
        #  that is not ascending)
        assert int((cp[:, 1] - cp[:, 0]).sum()) > 3072 and (np.diff(ci_in[starts[0] + cp[0, 0]:starts[0] + cp[0, 1]]) < 0).any()
    got = ecb.hapcsc_to_csr(torch.from_numpy(cp).cuda(), torch.from_numpy(ci_in).cuda(), E)
    for g, w in zip(got, csr):
        assert np.array_equal(g.cpu().numpy(), w)
    for g, w in zip(ecb.hapcsc_to_csr_host(cp, ci_in, E), csr):
        assert np.array_equal(g, w)
    dcp, dci = ecb.csr_to_hapcsc(*(torch.from_numpy(x).cuda() for x in csr), T, H)
    assert np.array_equal(dcp.cpu().numpy(), cp) and np.array_equal(dci.cpu().numpy(), ci)
    hcp, hci = ecb.csr_to_hapcsc_host(*csr, T, H)
    assert np.array_equal(hcp, cp) and np.array_equal(hci, ci)


def _count_only(csr, T, H):
    """The first call of ecb_csr_to_hapcsc_device: no outputs, the number of row indices there will be."""
    import torch
    lib = ecb.load()
    d = [torch.from_numpy(x).cuda() for x in csr]
    tot = C.c_uint64(0xDEAD)
    rc = lib.ecb_csr_to_hapcsc_device(0, len(csr[0]) - 1, T, H, ecb._dev_ptr(d[0]), ecb._dev_ptr(d[1]), ecb._dev_ptr(d[2]), None, None, C.byref(tot))
    assert rc == 0, lib.ecb_last_error(None)
    return tot.value


def test_count_only_call_of_csr_to_hapcsc(poison):
    """The count-only call adds the set bits of every mask into one word of the per-device pool: == numpy's popcount, on a pool that was
    just released (a fresh buffer), after a conversion and after an apply-mask (a buffer the calls before left behind), more than one
    block of k_cv_bits."""
    rng = np.random.default_rng(49)
    E, T, H = 3000, 500, 8
    csr = gt_checker.random_csr(rng, E, T, H)
    want = int(np.unpackbits(csr[2].view(np.uint8)).sum())
    assert len(csr[2]) > 2 * 256
    assert ecb.load().ecb_release_scratch(0) == 0
    assert _count_only(csr, T, H) == want
    ecb.csr_to_hapcsc_host(*csr, T, H)
    assert _count_only(csr, T, H) == want
    ecb.apply_mask(*csr, np.full(T, 0x55, np.uint32), H)
    assert _count_only(csr, T, H) == want
    small = tuple(x[:n] for x, n in zip(csr, (11, csr[0][10], csr[0][10])))
    assert _count_only(small, T, H) == int(np.unpackbits(small[2].view(np.uint8)).sum())


@pytest.mark.parametrize("n_ecs,n_loci", [(60, 40), (4097, 1000)], ids=["one-block", "blocks"])
def test_apply_mask_below_and_above_a_block(poison, n_ecs, n_loci):
    import torch
    rng = np.random.default_rng(50 + n_ecs)
    H = 8
    ip, ix, da = gt_checker.random_csr(rng, n_ecs, n_loci, H)
    assert (len(ix) < 1024) == (n_ecs == 60) and (len(ix) > 16_384) == (n_ecs != 60)
    mask = rng.integers(0, 1 << H, size=n_loci, dtype=np.int64).astype(np.uint32)
    exp = gt_checker.mask_csr(ip, ix, da, mask)
    tmg._same(ecb.apply_mask(ip, ix, da, mask, H), exp)
    dev = ecb.apply_mask(*[torch.from_numpy(a.view(np.int32)).cuda() for a in (ip, ix, da, mask)], H)
    tmg._same(dev, exp)


@pytest.mark.parametrize("nnz", [1023, 16_385])
def test_count_alignments_below_and_above_a_block(poison, nnz):
    """One sample, and three samples with weights (one column, and the sum of all), host and device entries."""
    import torch
    rng = np.random.default_rng(nnz)
    T, H = 3000, 8
    lens = rng.integers(0, 5, size=nnz)
    lens = lens[:int(np.searchsorted(np.cumsum(lens), nnz, side="right"))]
    lens = np.append(lens, nnz - lens.sum())
    ip, ix, da = tca._short_rows(rng, lens, T, H)
    da[rng.random(len(da)) < 0.05] = 0                                   # (zero masks: the second scan)
    E = len(lens)
    cols = [np.sort(rng.choice(E, size=k, replace=False)) for k in (E // 2, 0, E // 3)]
    N3 = (np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32), np.concatenate(cols).astype(np.int32),
          rng.integers(0, 1000, size=sum(len(c) for c in cols)).astype(np.int32))
    for N, sample in ((tca._one_sample(rng, E), None), (N3, None), (N3, 2)):
        exp = counts_checker.count(ip, ix, da, T, H, *N, sample=sample)
        tca._same(ecb.count_alignments(ip, ix, da, T, H, *N, sample=sample), exp)
        dev = ecb.count_alignments(*[torch.from_numpy(a).cuda() for a in (ip, ix, da)], T, H, *[torch.from_numpy(a).cuda() for a in N], sample=sample)
        tca._same(dev, exp)


@pytest.mark.parametrize("n_ecs", [150, 3000])
def test_combine_two_and_three_parts_with_overlapping_rows(poison, n_ecs):
    rng = np.random.default_rng(51 + n_ecs)
    hname = ["A", "B", "C"]
    names = ["t%03d" % i for i in range(60)]                             # (few targets: short rows meet again in the other parts)
    ms = [chk.random_bin(rng, n_ecs, names, hname, ["s1", "s2"], max_row=50),
          chk.random_bin(rng, n_ecs // 2, names, hname, ["s2", "s3"], max_row=50),
          chk.random_bin(rng, n_ecs, names, hname, ["s4"], max_row=50)]
    for m in ms[1:]:
        m.lengths = ms[0].lengths
    rows = [set((tuple(m.indicesA[a:z]), tuple(m.dataA[a:z])) for a, z in zip(m.indptrA[:-1], m.indptrA[1:])) for m in ms]
    assert rows[0] & rows[1] and rows[0] & rows[2]
    for sub in (ms[:2], ms):
        assert bin_utils.ecsave2_bytes(tmg._combine(sub)) == chk.merge_bytes(sub)


@pytest.mark.parametrize("L", [WAVE + 1, FOLD_TPB + 44])
def test_bundle_runs_across_a_wave_and_a_workgroup_of_the_fold(poison, L):
    """Runs of L loci that all fall into one group, started around the wave and workgroup boundaries of the fold (the construction of
    test_gpu_ecbundle.py::test_runs_on_the_wave_and_workgroup_boundaries_of_the_fold), and a random grouping."""
    F = FOLD_TPB
    T, H = F + L, 8
    groups = [[t] for t in range(F)] + [list(range(F, F + L))]
    starts = set()
    for B in (WAVE, FOLD_TPB):
        for d in (-1, 0, 1):
            starts.add((B + d) % FOLD_TPB)
            starts.add((B - L + d) % FOLD_TPB)
    rng = np.random.default_rng(L)
    rows, pos = [], 0
    for s in sorted(starts):
        n = (s - pos) % FOLD_TPB
        rows.append((np.arange(n), rng.integers(1, 1 << H, n)))
        rows.append((np.arange(F, F + L), 1 << rng.integers(0, H, L)))
        pos += n + L
    tb._agree(tb._m(rows, H, T), tb._names(F + 1), groups)
    m = chk.random_bin(rng, 800, tb._names(200, "t"), tb._names(4, "h"), ["s", "u"], max_row=150)
    groups = tb._grouping("mixed", rng, 200)
    tb._agree(m, tb._names(len(groups)), groups)


@pytest.mark.parametrize("E", [20, 5000])
def test_salmon_ecs_in_one_block_of_text_and_in_several(poison, E):
    rng = np.random.default_rng(52 + E)
    H = 4
    names = schk.target_names(150, ["h%d" % h for h in range(H)], rng)
    eff = rng.uniform(0, 5000, size=len(names))
    ptr, tid, counts = schk.random_ecs(rng, len(names), E, mean_k=6.0, long_every=50, long_k=(50, 400))
    section = schk.ec_section(ptr, tid, counts)
    assert (len(section) < 1024) == (E == 20) and (len(section) > 65_536) == (E != 20)
    lname, hname, col, hap = schk.number_names(names)
    got = ecb.salmon_ecs(section, E, col, hap, len(lname), len(hname))
    exp = schk.expected(names, eff, ptr, tid, counts)
    for g, e in zip(got, (exp[3], exp[4], exp[5], exp[7], exp[8])):
        assert np.array_equal(np.asarray(g, dtype=np.int64), np.asarray(e, dtype=np.int64))


# ---- the per-device pool: no call may depend on the call before ---------------------------------------------------------------------------
USERS = ("csr_to_hapcsc", "hapcsc_to_csr", "apply_mask", "count_alignments")
ORDER = (0, 1, 2, 3, 0, 2, 1, 3, 1, 0, 3, 2, 0)                          # every user right behind every other one, once
SIZES = (1.0, 0.1, 1.1, 1.3)                                              # dirty and smaller; within the eighth of slack; regrown


def _pool_cases():
    def make():
        from scipy import sparse
        rng = np.random.default_rng(53)
        T, H = 700, 6
        ip, ix, da = gt_checker.random_csr(rng, 9000, T, H, max_row=300)
        mask = rng.integers(0, 1 << H, size=T, dtype=np.int64).astype(np.uint32)
        full = int(ip[-1]) / 1.3
        out = {}
        for f in SIZES:
            E = int(np.searchsorted(ip, f * full, side="right")) - 1
            nnz = int(ip[E])
            csr = (ip[:E + 1].copy(), ix[:nnz].copy(), da[:nnz].copy())
            row = np.repeat(np.arange(E), np.diff(csr[0]))
            bits = (csr[2][:, None] >> np.arange(H)[None, :]) & 1
            k, h = np.nonzero(bits)
            _, csc = _hapcsc(E, T, H, row[k], csr[1][k].astype(np.int64), h)
            N = tca._one_sample(rng, E)
            out[f] = dict(E=E, csr=csr, csc=csc, N=N, masked=gt_checker.mask_csr(*csr, mask), counts=counts_checker.count(*csr, T, H, *N))
        return T, H, mask, out
    return _cached("pool", make)


def _run_user(user, case, T, H, mask, device):
    import torch
    up = (lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()) if device else (lambda a: a)   # noqa: E731
    down = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)   # noqa: E731
    csr, (cp, ci) = case["csr"], case["csc"]
    if user == "csr_to_hapcsc":
        got = ecb.csr_to_hapcsc(*map(up, csr), T, H) if device else ecb.csr_to_hapcsc_host(*csr, T, H)
        want = (cp, ci)
    elif user == "hapcsc_to_csr":
        got = ecb.hapcsc_to_csr(up(cp), up(ci), case["E"]) if device else ecb.hapcsc_to_csr_host(cp, ci, case["E"])
        want = csr
    elif user == "apply_mask":
        got = ecb.apply_mask(*map(up, csr), up(mask), H)
        want = case["masked"]
    else:
        got = ecb.count_alignments(*map(up, csr), T, H, *map(up, case["N"]))
        want = case["counts"]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.array_equal(np.asarray(down(g), dtype=np.int64), np.asarray(w, dtype=np.int64)), user


def test_pool_users_in_every_order_at_falling_and_rising_sizes_around_a_refused_call(poison):
    """The four users of the per-device pool behind each other -- every one right behind every other one -- while the size goes large,
    a tenth, 1.1 x (fits the pool's slack), 1.3 x (regrows), device and host entries in turn.  The pool is released before every such
    cycle of four, and the whole sequence runs four times with the users moved on by one, so every user meets every step of the cycle on a
    pool that the steps before left as they did.  In the middle a call that is refused (a malformed CSR: ECB_ERR_CONTRACT) leaves its
    outputs as they were, and the next call is right."""
    T, H, mask, cases = _pool_cases()
    assert {(a, b) for a, b in zip(ORDER, ORDER[1:])} == {(a, b) for a in range(4) for b in range(4) if a != b}
    nnz = [len(cases[f]["csr"][1]) for f in SIZES]
    assert nnz[1] * 9 < nnz[0] and nnz[0] < nnz[2] <= nnz[0] * 1.125 and nnz[3] > nnz[0] * 1.25
    lib = ecb.load()
    for rot, (k, u) in ((r, ku) for r in range(4) for ku in enumerate(ORDER)):
        if k % 4 == 0:
            assert lib.ecb_release_scratch(0) == 0
        _run_user(USERS[(u + rot) % 4], cases[SIZES[k % 4]], T, H, mask, device=(k + rot) % 2 == 0)
        if k == 6 and rot == 0:
            c = cases[1.0]
            ip = c["csr"][0].copy()
            ip[10], ip[11] = ip[11] + 1, ip[10]                          # (falling row pointers)
            arrs = [np.ascontiguousarray(a, dtype=np.int32) for a in (ip, c["csr"][1], c["csr"][2]) + tuple(c["N"])]
            outs = [np.full((H, T), 7, np.int64), np.full((H, T), 7, np.int64), np.full(T, 7, np.int64)]
            ptr = lambda v: v.ctypes.data_as(C.c_void_p)   # noqa: E731
            rc = lib.ecb_count_alignments(0, c["E"], T, H, len(arrs[1]), ptr(arrs[0]), ptr(arrs[1]), ptr(arrs[2]), 1, len(arrs[4]), ptr(arrs[3]),
                                          ptr(arrs[4]), ptr(arrs[5]), -1, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]))
            assert rc == CONTRACT, (rc, lib.ecb_last_error(None))
            assert all((o == 7).all() for o in outs)
