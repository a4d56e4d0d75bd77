"""The exactness pass -- ``ecb_verify_device``, ``ecb_verify_device_tiled``, ``ECB_F_VERIFY`` (``EcBuilder(verify=True)``,
``ALNTOOLS_VERIFY=1``) -- is the referee the rest of the suite trusts whenever it asserts ``verify_device(...)[0] == 0``.  Here the
referee itself is checked: a stream S is pushed, streams S' that differ from it in known reads are verified against the handle, and the
count that comes back must be the one ``verify_checker.misplaced`` (plain numpy, pinned by ``test_verify_checker.py``) derives -- exactly,
one changed read at a time on every compare path (the quick compare on one pair and on the inline pairs, ``cmp.full`` and the arena walk
for keys beyond INL = 5 pairs, ``k_slow`` with the read's table in LDS and in global scratch) and for every way two target sets can
differ, then many reads at once, as three arrays and as tiles, after the table grew and after host pushes; the pass must leave the handle
as it found it.  Then the handle that checks itself after every batch: every way in must give the C oracle's answer with no error.

Every stream here obeys the tuple contract.  ``ECB_ERR_VERIFY`` (-9) cannot be provoked from outside without a bug in the library: that
return of ``process_batch`` is covered by code reading only."""
import json
import os

import numpy as np
import pytest

from alntools_amd import bam_utils, bamio, ecb
from oracle import ec_oracle as orc

import test_gpu_multisample as tm
import test_gpu_poisoned_scratch as tp
import test_gpu_thresholds as th
from test_gpu_parity import _check
from verify_checker import COUNTED, KINDS, NOT_COUNTED, misplaced, perturb

pytestmark = pytest.mark.gpu

T, H = 20_000, 8
SMALL = tp.SMALL
# records per read of every class (``test_threshold_constants.py`` pins INL, CMAX, WT and SLOW_LDS): a -- one pair; b -- the inline pairs;
# c -- pairs in the arena, the read stays in the pass; d -- up to 300: k_slow in LDS when the read is open at a tile's end; d1025 = 2 WT + 1:
# covers a whole tile, so always deferred, table in LDS; e -- 2 x records > SLOW_LDS: always deferred, table in global scratch
SIZES = {"a": (1,), "b": (2, 3, 5), "c": (6, 7, 40, th.CMAX_STD), "d": (81, 150, 300), "d1025": (2 * th.WT + 1,), "e": (th.SLOW_LDS // 2 + 1,)}
CLASSES = tuple(SIZES)
AT_THE_ENDS = {"a": 1, "b": 5, "c": 40, "d": 300, "d1025": SIZES["d1025"][0], "e": SIZES["e"][0]}       # the size a class sends to the stream's first and last place
N_VARIANTS = len(CLASSES)
#: the (class, kind) pairs of the one-at-a-time case: one record has nothing behind its head; the highest and the lowest locus are the last
#: pair in the arena and the first inline pair only where a key has pairs in the arena
PAIRS = ({("a", k) for k in ("hap", "locus")} | {("b", k) for k in KINDS if not k.startswith("hap_")} |
         {(c, k) for c in ("c", "d", "d1025", "e") for k in KINDS})


def _flags(rng, n, some=False):
    """Flag 0x4 on a tenth of the records behind the head; ``some``: at least one of them invalid, the second and the last record valid."""
    f = np.where(rng.random(n) < 0.1, 0x4, 0).astype(np.uint32)
    if some and n >= 3:
        f[n // 2] = 0x4
        f[1] = f[-1] = 0
    f[0] = 0
    return f


def _class_read(rng, n):
    loci, haps = th._distinct(rng, n, T, H)
    return loci, haps, _flags(rng, n, some=True)


_CACHE = {}


def _variant(v):
    """Base stream number v: about 3 000 short reads (``th._fill``) with three reads of every size of every class among them; its first read
    is of class v, its last of class v + 2 -- over the variants every class is first once and last once.  -> dict(t, cls [class of every
    read or None], exp [the C oracle], n_long [reads of 1 025 and 2 049 records], many [S' with a tenth of the reads changed], many_bad)."""
    if v in _CACHE:
        return _CACHE[v]
    rng = np.random.default_rng(600 + v)
    fill = [(lo, ha, _flags(rng, len(lo))) for lo, ha in th._fill(rng, 15_000, T, H)]
    body = [(None, r) for r in fill]
    special = [(c, n) for c in CLASSES for n in SIZES[c] for _ in range(3)]
    for k in rng.permutation(len(special)):
        c, n = special[k]
        body.insert(int(rng.integers(0, len(body) + 1)), (c, _class_read(rng, n)))
    first, last = CLASSES[v], CLASSES[(v + 2) % N_VARIANTS]
    body = [(first, _class_read(rng, AT_THE_ENDS[first]))] + body + [(last, _class_read(rng, AT_THE_ENDS[last]))]
    t = th._stream([r for _, r in body])
    cls = [c for c, _ in body]
    n = len(t["read_id"])
    assert n < 60_000 and 2900 < len(body) and int(t["locus"].max()) < T and orc.tuples_valid(t["hapflag"][np.flatnonzero(np.diff(t["read_id"])) + 1]).all()
    n_inv, behind = int((~orc.tuples_valid(t["hapflag"])).sum()), n - len(body)
    assert 0.08 * behind < n_inv < 0.12 * behind                      # (a tenth of the records behind the heads)
    lens = np.bincount(t["read_id"].astype(np.int64))
    out = dict(t=t, cls=cls, exp=th._oracle(t, H), n_reads=len(body), n_long=int(((lens == SIZES["d1025"][0]) | (lens == SIZES["e"][0])).sum()))
    assert out["n_long"] >= 6 and out["exp"]["n_reads"] == len(body)
    # many at once: a tenth of the reads and the two at the ends, each changed in one way picked at random among those it has the records for
    chosen = set(rng.choice(len(body), size=len(body) // 10, replace=False).tolist()) | {0, len(body) - 1}
    t2, counted = t, 0
    for r in sorted(chosen):
        for kind in rng.permutation(KINDS):
            p = perturb(t2, r, str(kind), T, H)
            if p is not None:
                t2, counted = p, counted + (kind in COUNTED)
                break
    bad = misplaced(t, t2, H)
    assert int(bad.sum()) == counted and 0 < counted < len(body) and not bad[sorted(set(range(len(body))) - chosen)].any()
    out["many"], out["many_bad"] = t2, counted
    _CACHE[v] = out
    return out


def _target(S, v, c, kind):
    """The read of class c that case (c, kind) of variant v changes, and S' -- the stream's first or last read where that is of class c,
    else one in the middle, the sizes of the class taken in turn."""
    reads = [r for r, x in enumerate(S["cls"]) if x == c]
    mid = [r for r in reads if 0 < r < S["n_reads"] - 1]
    turn = (KINDS.index(kind) + v) % len(mid)
    order = [r for r in reads if r in (0, S["n_reads"] - 1)] + mid[turn:] + mid[:turn]
    for r in order:
        t2 = perturb(S["t"], r, kind, T, H)
        if t2 is not None:
            return r, t2
    return None, None


def _up(a):
    import torch
    return torch.from_numpy(a.view(np.int32)).cuda()


def _changed(S, d, t2):
    """Device arrays of S': only what differs from S is uploaded."""
    return [d[0]] + [d[k] if t2[name] is S["t"][name] else _up(t2[name]) for k, name in ((1, "locus"), (2, "hapflag"))]


# ---- ecb_verify_device / ecb_verify_device_tiled against the checker ------------------------------------------------------------------------
@pytest.mark.parametrize("v", range(N_VARIANTS))
def test_one_changed_read_at_a_time_on_every_compare_path(v):
    """One handle, S pushed once; for every class and every kind that applies to it an S' with exactly one read changed: 1 for the seven
    kinds that change the read's set, 0 for the two that change its records only, and each time the checker's count.  Only a count comes
    back: single reads keep a miss on one path from cancelling against a false alarm on another.  The reads of 1 025 and 2 049 records
    also as tiles.  The second figure: at least the reads of those two sizes, every time."""
    S = _variant(v)
    t, n = S["t"], len(S["t"]["read_id"])
    d = th._dev(t)
    ran, wrong, at_ends = set(), [], set()
    with ecb.EcBuilder(T, H, **SMALL) as b:
        b.push_device(*d)
        _check(b.export(), b.finalize(), S["exp"])
        clean = b.verify_device(*d)
        assert clean[0] == 0 and clean[1] >= S["n_long"], clean
        for c, kind in sorted(PAIRS):
            r, t2 = _target(S, v, c, kind)
            assert t2 is not None, (c, kind)
            m = misplaced(t, t2, H)
            want = 1 if kind in COUNTED else 0
            assert int(m.sum()) == want and bool(m[r]) == bool(want), (c, kind, r)
            d2 = _changed(S, d, t2)
            bad, long_ = b.verify_device(*d2)
            print("variant %d class %s kind %s read %d (%d records): bad %d (reference %d), long %d" %
                  (v, c, kind, r, int((t["read_id"] == r).sum()), bad, want, long_))
            if bad != want or long_ < S["n_long"]:
                wrong.append((c, kind, r, bad, want, long_))
            if c in ("d1025", "e") and kind in ("hap", "dup"):
                tb, tl = b.verify_device_tiled(ecb.tile_tuples(*d2), n)
                print("  ... as tiles: bad %d, long %d" % (tb, tl))
                if tb != want or tl < S["n_long"]:
                    wrong.append((c, kind, r, "tiled", tb, want, tl))
            ran.add((c, kind))
            if r in (0, S["n_reads"] - 1):
                at_ends.add((c, r == 0))
        assert not wrong, wrong
        assert b.verify_device(*d) == clean                          # (and nothing of all that stayed behind)
    assert ran == PAIRS
    assert at_ends == {(CLASSES[v], True), (CLASSES[(v + 2) % N_VARIANTS], False)}


def test_the_variants_put_every_class_first_once_and_last_once():
    firsts = [_variant(v)["cls"][0] for v in range(N_VARIANTS)]
    lasts = [_variant(v)["cls"][-1] for v in range(N_VARIANTS)]
    assert sorted(firsts) == sorted(lasts) == sorted(CLASSES)
    for v in range(N_VARIANTS):
        sizes = np.bincount(_variant(v)["t"]["read_id"].astype(np.int64))
        for c in CLASSES:
            for s in SIZES[c]:
                assert int((sizes == s).sum()) >= 3, (v, c, s)


@pytest.mark.parametrize("v", range(N_VARIANTS))
def test_many_changed_reads_at_once_as_arrays_and_as_tiles_and_the_pass_only_reads(v):
    """A tenth of the reads and the first and the last, each changed in one way: the checker's count through ``verify_device`` and
    through ``tile_tuples`` + ``verify_device_tiled``.  After passes that reported mismatches finalize, export and export_read_ec are what
    they were (the C oracle's), and S verifies clean again with the same reads on the long path."""
    S = _variant(v)
    t, t2, want, n = S["t"], S["many"], S["many_bad"], len(S["t"]["read_id"])
    d = th._dev(t)
    d2 = _changed(S, d, t2)
    with ecb.EcBuilder(T, H, **SMALL) as b:
        b.push_device(*d)
        s0 = b.finalize()
        _check(b.export(), s0, S["exp"])
        ec0 = b.export_read_ec()
        clean = b.verify_device(*d)
        assert clean[0] == 0 and clean[1] >= S["n_long"], clean
        bad, long_ = b.verify_device(*d2)
        print("variant %d: bad %d (reference %d of %d reads), long %d" % (v, bad, want, S["n_reads"], long_))
        assert bad == want and long_ >= S["n_long"]
        tb, tl = b.verify_device_tiled(ecb.tile_tuples(*d2), n)
        print("  ... as tiles: bad %d, long %d" % (tb, tl))
        assert tb == bad == want and tl >= S["n_long"]
        assert b.finalize() == s0
        _check(b.export(), s0, S["exp"])
        assert np.array_equal(b.export_read_ec(), ec0)
        assert b.verify_device(*d) == clean
        tb, tl = b.verify_device_tiled(ecb.tile_tuples(*d), n)
        assert tb == 0 and tl >= S["n_long"]


def _cuts(t, pieces):
    """Record indices that cut the stream into about ``pieces`` batches of whole reads, each starting on 16 bytes."""
    heads = np.concatenate(([0], np.flatnonzero(np.diff(t["read_id"])) + 1))
    heads = heads[heads % 4 == 0]
    n = len(t["read_id"])
    inner = sorted({int(heads[np.searchsorted(heads, k * n // pieces)]) for k in range(1, pieces)} - {0})
    assert len(inner) >= pieces - 2
    return [0] + inner + [n]


@pytest.mark.parametrize("how", ["device", "host777"])
def test_after_the_table_grew_and_after_host_pushes(how):
    """``ec_capacity=64`` (1 024 slots, kept half full): the table grows and read_slot is remapped between the batches -- five device
    batches of whole reads, or host batches of 777 records (reads carried over their ends) -- and one pass over the device copy of the
    whole stream then finds S clean and in S' the checker's count."""
    S = _variant(1)
    t, t2, want = S["t"], S["many"], S["many_bad"]
    d = th._dev(t)
    n = len(t["read_id"])
    with ecb.EcBuilder(T, H, ec_capacity=64, arena_capacity=1 << 24) as b:
        if how == "device":
            c = _cuts(t, 5)
            for a, z in zip(c[:-1], c[1:]):
                b.push_device(*(x[a:z] for x in d))
        else:
            for a in range(0, n, 777):
                b.push(*(t[k][a:a + 777] for k in ("read_id", "locus", "hapflag")))
            b.counters()                                             # (the read the last push left open goes in)
        assert b.table_sizes()[0] == len(S["exp"]["count"]) > 1024
        clean = b.verify_device(*d)
        assert clean[0] == 0 and clean[1] >= S["n_long"], clean
        bad, long_ = b.verify_device(*_changed(S, d, t2))
        print("%s: bad %d (reference %d), long %d" % (how, bad, want, long_))
        assert bad == want and long_ >= S["n_long"]
        _check(b.export(), b.finalize(), S["exp"])
        assert b.verify_device(*d) == clean


# ---- the handle that checks itself (ECB_F_VERIFY) --------------------------------------------------------------------------------------------
T3 = 4000


def _self_stream():
    """The short stream of ``test_gpu_poisoned_scratch.py`` (3 000 reads of up to 12 records) with four reads of 1 025 and one of 2 049
    distinct loci among them, one of them first and one last (more loci than that stream's 2 000: the handles here are made for 4 000)."""
    def make():
        t0, _, H0, _ = tp._short_stream()
        rng = np.random.default_rng(70)
        parts = np.split(np.arange(len(t0["read_id"])), np.flatnonzero(np.diff(t0["read_id"])) + 1)
        reads = [(t0["locus"][p], t0["hapflag"][p] >> 16, t0["hapflag"][p] & 0xFFFF) for p in parts]
        for at, L in ((len(reads), 1025), (2200, 1025), (1500, 2049), (700, 1025), (0, 1025)):
            reads.insert(at, th._distinct(rng, L, T3, H0))
        t = th._stream(reads)
        t["pos"] = rng.integers(0, (1 << 31) - 1, size=len(t["read_id"])).astype(np.int32)
        return t, H0, th._oracle(t, H0)
    return tp._cached("self-checking", make)


def _push(b, t, d, how):
    n = len(t["read_id"])
    pos = b.track_ranges
    if how == "host":
        b.push(t["read_id"], t["locus"], t["hapflag"], t["pos"] if pos else None)
    elif how == "host777":
        for a in range(0, n, 777):
            b.push(*(t[k][a:a + 777] for k in ("read_id", "locus", "hapflag") + (("pos",) if pos else ())))
        b.counters()                                                 # (the carried read goes in)
    elif how == "device":
        b.push_device(*d[:4 if pos else 3])
    elif how == "device5":                                           # (the later batches verify with the read id before them)
        c = _cuts(t, 5)
        for a, z in zip(c[:-1], c[1:]):
            b.push_device(*(x[a:z] for x in d[:4 if pos else 3]))
    elif how == "tiled":
        b.push_device_tiled(ecb.tile_tuples(*d[:3]), n)
    else:
        raise ValueError(how)


def _dev4(t):
    import torch
    return th._dev(t) + [torch.from_numpy(t["pos"]).cuda()]


def _plain_sizes(t, Hn):
    def make():
        with ecb.EcBuilder(T3, Hn, **SMALL) as b:
            b.push(t["read_id"], t["locus"], t["hapflag"])
            return b.finalize()
    return tp._cached("self-checking-plain", make)


@pytest.mark.parametrize("how", ["host", "host777", "device", "device5", "tiled", "parked"])
def test_self_checking_handle_gives_the_oracles_answer_through_every_push(how):
    """``verify=True``: every batch is verified behind its push, and no way in may trip it or change the result.  ``parked``:
    ``ec_capacity=64``, one device push -- the launch parks, the table grows and the batch is relaunched before its pass."""
    t, Hn, exp = _self_stream()
    d = _dev4(t)
    kw = dict(SMALL, ec_capacity=64) if how == "parked" else SMALL
    with ecb.EcBuilder(T3, Hn, verify=True, **kw) as b:
        _push(b, t, d, "device" if how == "parked" else how)
        s = b.finalize()
        _check(b.export(), s, exp)
        assert s == _plain_sizes(t, Hn)
        ec = b.export_read_ec()
        assert len(ec) == exp["n_reads"] and np.array_equal(np.bincount(ec, minlength=s["n_ecs"]), exp["count"])
        if how == "parked":
            assert b.table_sizes()[0] > 1024
        assert b.verify_device(*d[:3])[0] == 0


@pytest.mark.parametrize("compilation", sorted(th.COMPILATIONS))
def test_self_checking_handle_through_every_compilation(compilation, monkeypatch):
    """Every compilation of the stream kernel forced in turn, hinted where its row says so (the hinted handle takes its last read id from
    the counters, which the pass's launch has gone over by then): the oracle's answer, and ``profile_kernel`` names the kernel that pushed,
    not the pass."""
    t, Hn, exp = _self_stream()
    env, hinted, kernel = th.COMPILATIONS[compilation]
    th._force(monkeypatch, env)
    d = _dev4(t)
    for how in ("device", "device5", "tiled", "host777"):
        with ecb.EcBuilder(T3, Hn, verify=True, **SMALL) as b:
            if hinted:
                b.hint_reads(exp["n_reads"])
            _push(b, t, d, how)
            assert b.profile_kernel().startswith(kernel), (how, b.profile_kernel())
            s = b.finalize()
            _check(b.export(), s, exp)
            assert s == _plain_sizes(t, Hn), how


def test_self_checking_handle_reset_and_a_shorter_stream():
    """``ecb_reset`` fills read_slot with 0xFF on such a handle; a shorter stream on the same handle, from the device and from the host."""
    t, Hn, exp = _self_stream()
    d = _dev4(t)
    z = int(np.searchsorted(t["read_id"], 1000))
    z -= z % 4
    while t["read_id"][z] == t["read_id"][z - 1]:
        z -= 4
    short = {k: t[k][:z] for k in ("read_id", "locus", "hapflag")}
    exp_short = th._oracle(short, Hn)
    assert 500 < exp_short["n_reads"] < 1001
    with ecb.EcBuilder(T3, Hn, verify=True, **SMALL) as b:
        b.push_device(*d[:3])
        _check(b.export(), b.finalize(), exp)
        b.reset()
        b.push_device(*(x[:z] for x in d[:3]))
        _check(b.export(), b.finalize(), exp_short)
        assert b.verify_device(*(x[:z] for x in d[:3]))[0] == 0
        b.reset()
        for a in range(0, z, 777):
            b.push(*(short[k][a:a + 777] for k in ("read_id", "locus", "hapflag")))
        _check(b.export(), b.finalize(), exp_short)
        b.reset()
        b.push(t["read_id"], t["locus"], t["hapflag"])
        _check(b.export(), b.finalize(), exp)


@pytest.mark.parametrize("how", ["host777", "device5", "device"])
def test_self_checking_handle_leaves_the_ranges_alone(how):
    """``track_ranges=True`` with positions: the pass runs between the batches' range kernels and stages its own cold block over theirs;
    export_ranges and export_range_minmax must be those of the same handle without the flag."""
    t, Hn, exp = _self_stream()
    d = _dev4(t)
    got = []
    for verify in (False, True):
        with ecb.EcBuilder(T3, Hn, track_ranges=True, verify=verify, **SMALL) as b:
            _push(b, t, d, how)
            assert b.profile_kernel() == "ks_std::k_stream<false, true>"
            _check(b.export(), b.finalize(), exp)
            got.append((b.export_ranges(),) + b.export_range_minmax())
    for plain, checked in zip(*got):
        assert np.array_equal(plain, checked)
    valid = orc.tuples_valid(t["hapflag"])
    slot = t["locus"].astype(np.int64) * Hn + ((t["hapflag"].astype(np.int64) >> 16) & 0xFF)
    mn = np.full(T3 * Hn, np.iinfo(np.int32).max, np.int64)
    np.minimum.at(mn, slot[valid], t["pos"].astype(np.int64)[valid])
    assert np.array_equal(got[1][1].reshape(-1), mn)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("tpl,cell,fil", [([0], [0], [0]), ([3], [tm.MAX_CELLS - 1], [1023]), ([0, 1], [1, 0], [0, 0]), ([0, 0, 1], [0, 1, 1], [0, 1, 1])],
                         ids=["one-read", "one-read-top-meta", "two-cells", "two-cells-two-files"])
def test_self_checking_multisample_handle(tpl, cell, fil, device):
    """``multisample=True``: cells through push_cells as ``test_gpu_multisample.py::test_smallest_inputs`` takes them; the triples are
    those of the handle without the flag (and the stream's own expectation)."""
    st = tm.Stream(tpl, cell, fil)
    got = []
    for verify in (False, True):
        with ecb.EcBuilder(st.n_loci, tm.H, multisample=True, verify=verify) as b:
            tm._push(b, st, device)
            tm._check_built(b, st, st.expected())
            got.append((b.export_pairs(), b.export()))
    for k in got[0][0]:
        assert np.array_equal(got[0][0][k], got[1][0][k]), k
    for k in got[0][1]:
        assert np.array_equal(got[0][1][k], got[1][1][k]), k


def test_alntools_verify_writes_the_same_bin(golden_dir, tmp_path, monkeypatch):
    """``ALNTOOLS_VERIFY=1``: ``bam_utils.convert`` makes its handle with ``verify=True`` and writes the bytes it writes without."""
    g = json.load(open(os.path.join(golden_dir, "g1_edge.json")))
    bam = str(tmp_path / g["sample"])
    bamio.write_bam(bam, [tuple(r) for r in g["references"]], [tuple(r) for r in g["records"]])
    seen, real = [], bam_utils.EcBuilder

    def spy(*a, **kw):
        seen.append(kw.get("verify"))
        return real(*a, **kw)
    monkeypatch.setattr(bam_utils, "EcBuilder", spy)
    monkeypatch.delenv("ALNTOOLS_GPUS", raising=False)
    outs = []
    for on in (False, True):
        if on:
            monkeypatch.setenv("ALNTOOLS_VERIFY", "1")
        else:
            monkeypatch.delenv("ALNTOOLS_VERIFY", raising=False)
        out, rng = str(tmp_path / ("o%d.bin" % on)), str(tmp_path / ("o%d.range" % on))
        bam_utils.convert(bam, out, None, range_filename=rng)
        outs.append((open(out, "rb").read(), open(rng).read()))
    assert seen == [False, True]
    assert outs[0] == outs[1]
    assert outs[1][0] == open(os.path.join(golden_dir, "g1_edge.bin"), "rb").read()
    assert outs[1][1] == open(os.path.join(golden_dir, "g1_edge.range.txt")).read()
