"""Every break of the tuple contract (``include/ecb.h``; the table in DESIGN.md section 2) that the library refuses today, at every place
where the stream kernel could lose sight of it, through every way into the library: refused with ECB_ERR_CONTRACT and the text of the table,
at the call the table names; the handle is then a refused run until ``ecb_reset``; and after the reset the same handle takes the unbroken
stream and gives the C oracle's result bit for bit -- A, N, the counters, the EC of every read, and the ranges or the (EC, cell, file)
triples where the handle keeps them -- which is what shows that the refused stream wrote nowhere it should not have.  The legal near misses
-- a head on each of the same places, a read that ends on every edge, the same indices out of range in records that do not pass the
filter, the ignored bits 14 - 15 -- are accepted and equal the oracle, so a check that is too strict fails here too.

The streams, breaks and places are ``contract_streams.py``'s; ``test_contract_streams.py`` proves on the CPU what each of them is.  Which
breaks may run at all follows from the table: each is refused before an address depends on the broken word, or every address that depends
on it stays in the library's own memory (a locus below 2^26 - 1 and a haplotype below 32 travel as data until the emit looks at them).
NOT run here, because the kernel does not refuse them and reading cannot show them safe: run-counter steps that cancel within one lane's
four records, and locus 0xFFFFFFFF in a passing record (``contract_streams.py``: the open hole)."""
import numpy as np
import pytest

from alntools_amd import ecb
from oracle import c_oracle
from oracle import ec_oracle as orc

import contract_streams as cs
import refusal_streams as rs
import test_gpu_thresholds as th
from test_gpu_parity import _check

pytestmark = pytest.mark.gpu

CONTRACT, STATE = -5, -6
RUN_TEXT = "read_id run counter violates the tuple contract (see ecb.h)"
INDEX_TEXT = "locus or haplotype index out of range in a valid record"
SMALL = dict(ec_capacity=1 << 12, arena_capacity=1 << 24)
CELLS, FILES = 8, 2

# way in -> (environment, arguments of the handle, the compilation ecb_profile_kernel must report)
WAYS = {
    "device": (("ECB_NO_PAR",), {}, "ks_std::k_stream<false, false>"),
    "tiled": (("ECB_NO_PAR",), {}, "ks_std::k_stream<false, false>"),
    "host": (("ECB_NO_PAR",), {"max_batch_records": 4096}, "ks_std::k_stream<false, false>"),        # (a call's records are one window: the cuts are _push's)
    "par": (("ECB_FORCE_PAR",), {}, "ks_par::k_stream<false, false>"),
    "short": (("ECB_FORCE_SHORT",), {}, "ks_short::k_stream<false, false>"),
    "ranges": (("ECB_NO_PAR",), {"track_ranges": True}, "ks_std::k_stream<false, true>"),
    "multisample": (("ECB_NO_PAR",), {"multisample": True}, "ks_std::k_stream<false, false>"),
}

_EXP = {}
HIP = -2


def _a_hip_error_ends_the_session(test):
    """A HIP error (a fault among them) is no test failure to run on from: nothing more is started on the card.  This ends the whole session,
    on an error that is no fault -- out of memory -- too: the cautious side.  (A decorator of this module, not a hook: the project's conftest
    is not this module's to change.)"""
    import functools

    @functools.wraps(test)
    def run(*a, **kw):
        try:
            return test(*a, **kw)
        except ecb.EcbError as e:
            if e.code == HIP:
                pytest.exit("HIP error, session ended: %s" % e, returncode=3)
            raise
    return run


def _meta(n_reads):
    r = np.arange(n_reads)
    return (cs._rnd(r, 91, CELLS) | (cs._rnd(r, 92, FILES) << 22)).astype(np.uint32)


def _expected(kind, which):
    """The C oracle's result of a legal stream, made once: with the EC of every read, the ranges and the (EC, cell, file) triples."""
    if (kind.name, which) not in _EXP:
        t = kind.stream(which)
        exp = c_oracle.ec_from_tuples(t["read_id"], t["locus"], t["hapflag"], kind.n_haps, threads=2)
        row = {tuple(zip(exp["indices"][a:z].tolist(), exp["data"][a:z].tolist())): e
               for e, (a, z) in enumerate(zip(exp["indptr"][:-1], exp["indptr"][1:]))}
        exp["read_ec"] = np.array([row[k] for k in rs.read_keys(t)], np.int32)
        exp["range"] = orc.ec_from_tuples(t["read_id"], t["locus"], t["hapflag"], kind.n_loci, kind.n_haps, pos=t["pos"])["range"]
        meta = _meta(exp["n_reads"]).astype(np.int64)
        key = (exp["read_ec"].astype(np.int64) << 32) | ((meta & ((1 << 22) - 1)) << 10) | (meta >> 22)          # (EC, cell, file): the order of the triples
        uk, first, count = np.unique(key, return_index=True, return_counts=True)
        exp["pairs"] = dict(ec=uk >> 32, cell=(uk >> 10) & ((1 << 22) - 1), file=uk & 1023, count=count.astype(np.int64), first=first.astype(np.int64))
        for v in list(exp.values()) + list(exp["pairs"].values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _EXP[kind.name, which] = exp
    return _EXP[kind.name, which]


def _dev(t):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(t[k]).view(np.int32)).cuda() for k in ("read_id", "locus", "hapflag", "pos")]


def _push(b, way, t, cut=None):
    """The stream through the way in.  host: in two calls, the first of which ends with record ``cut`` -- a head, so that the batch the library
    makes of the second call starts there -- and the counters asked for, which sends the read the host push left open."""
    if way == "host":
        c = len(t["read_id"]) // 2 if cut is None else cut + 1
        for sl in (slice(0, c), slice(c, None)):
            b.push(t["read_id"][sl], t["locus"][sl], t["hapflag"][sl])
        b.counters()
        return
    d = _dev(t)
    if way == "tiled":
        b.push_device_tiled(ecb.tile_tuples(*d[:3]), len(t["read_id"]))
    else:
        b.push_device(*(d if way == "ranges" else d[:3]))


def _accepted(b, way, kind, t, exp):
    """A legal stream into the handle: == the oracle.  Leaves the handle reset."""
    _push(b, way, t)
    kernel = b.profile_kernel()
    if way == "multisample":
        b.push_cells(_meta(exp["n_reads"]), 0)
    s = b.finalize()
    out = b.export()
    assert b.counters() == (exp["n_all"], exp["n_valid"], exp["n_reads"]) and s["n_reads"] == exp["n_reads"]
    assert np.array_equal(b.export_read_ec(), exp["read_ec"])
    if way == "multisample":
        assert s["n_ecs"] == len(exp["count"]) and s["all_alignments"] == exp["n_all"] and s["valid_alignments"] == exp["n_valid"]
        for k, e in (("indptrA", "indptr"), ("indicesA", "indices"), ("dataA", "data")):
            assert np.array_equal(out[k], exp[e]), k
        got = b.export_pairs()
        for k, v in exp["pairs"].items():
            assert np.array_equal(got[k], v), k
    else:
        _check(out, s, exp)
    if way == "ranges":
        assert np.array_equal(b.export_ranges(), exp["range"])
    b.reset()
    return kernel


def _refused(b, way, u, text, at, cut=None):
    """The broken stream ``u``: ECB_ERR_CONTRACT with ``text``, from the push (at == 'push') or from finalize at the latest; then a refused
    run -- finalize, the counters and a further push answer ECB_ERR_STATE and name the refusal -- until ecb_reset."""
    with pytest.raises(ecb.EcbError) as e:
        _push(b, way, u, cut)
        assert at == "finalize", "accepted by the push"
        b.finalize()
    first = (b._lib.ecb_last_error(b._h) or b"").decode()
    if e.value.code == HIP:
        raise e.value
    assert e.value.code == CONTRACT and text in first, str(e.value)
    for call in (b.finalize, b.counters, lambda: _push(b, way, u, cut)):
        with pytest.raises(ecb.EcbError) as e:
            call()
        assert e.value.code == STATE and first in str(e.value) and "(%d: " % CONTRACT in str(e.value) and "ecb_reset" in str(e.value), str(e.value)
    b.reset()
    assert (b._lib.ecb_last_error(b._h) or b"") == b""


def _handle(kind, way, monkeypatch):
    env, args, kernel = WAYS[way]
    th._force(monkeypatch, env)
    b = ecb.EcBuilder(kind.n_loci, kind.n_haps, **dict(SMALL, **args))
    if kind.hinted:
        b.hint_reads(max(kind.stream(w)["n_reads"] for w in (None, 0, 1, 2, 3)) + 2)      # (room for the breaks that end one read later)
    return b, kernel


def _index_refused_at(way, field, value, in_giant):
    """where an index out of range in a passing record is refused.  The stream kernel sees a locus whose key would not
    fit KBITS (26 bits; 25 in ks_short), locus 0xFFFFFFFF, a haplotype of 32 or more (8 or more where the masks are bytes) and bits 24 - 31;
    k_slow holds every record of a read it is given to n_loci and n_haplotypes; everything else waits for the emit."""
    kbits, hmax = (25, 8) if way == "short" else (26, 32)
    if in_giant or field == "bit":
        return "push"
    if field == "locus":
        return "push" if value == 0xFFFFFFFF or value + 1 >= 1 << kbits else "finalize"
    return "push" if value >= hmax else "finalize"


COMBOS = [("mid", w) for w in ("device", "tiled", "host", "par", "ranges", "multisample")] + [("long", w) for w in ("device", "tiled", "par")] + \
         [("short", "short"), ("giant", "device"), ("giant", "host")]


@pytest.mark.parametrize("name,way", COMBOS, ids=["%s-%s" % c for c in COMBOS])
@_a_hip_error_ends_the_session
def test_run_counter_breaks_are_refused_at_the_push(name, way, monkeypatch):
    """Every run-counter break (all of them at every place for the plain device push of ``mid`` and for the host pushes; elsewhere "+2 -2" at
    every place and each other break at a quarter of the places), and after each the base stream through the same handle.  host: the first
    call ends with the last head at or before the break, so the batch the library forms next starts there and the break sits in its first
    lane groups.  The lanes of that batch count from its own first record: a break whose steps cancel within one of THOSE groups of four is
    the open hole too, and is left out."""
    kind = cs.KINDS[name]
    b, kernel = _handle(kind, way, monkeypatch)
    with b:
        seen = set()
        for label, brk, which, x in cs.run_counter_cases(kind, every=(name, way) == ("mid", "device") or way == "host", refused_today=True):
            t = kind.stream(which)
            u, _ = brk(t, x)
            heads = cs.heads_of(t)
            cut = int(heads[heads <= x][-1])
            if way == "host" and brk.width is not None and cs.in_one_lane(x + brk.at - cut, brk.width):
                continue                                # (the batch starts at `cut`: in ITS lanes the steps cancel -- the open hole)
            _refused(b, way, u, RUN_TEXT, "push", cut=cut)
            seen.add(_accepted(b, way, kind, t, _expected(kind, which)))
        assert len(seen) == 1 and seen.pop().startswith(kernel)


@pytest.mark.parametrize("name,way", COMBOS, ids=["%s-%s" % c for c in COMBOS])
@_a_hip_error_ends_the_session
def test_near_misses_and_filtered_records_are_accepted(name, way, monkeypatch):
    """The four near-miss streams (a head on every place, a read ending on every edge), and every index break in a record that does not
    pass the filter: accepted, == the oracle (the latter: == the base stream's result)."""
    kind = cs.KINDS[name]
    b, kernel = _handle(kind, way, monkeypatch)
    with b:
        for j in range(4):
            assert _accepted(b, way, kind, kind.near_miss[j], _expected(kind, j)).startswith(kernel)
        t = kind.base
        for place in ("lane17+0", "short tile+1") + (("giant+0",) if kind.giant else ()):
            x = cs.a_filtered_record(t, kind.places()[place])
            for label, fn, _, _, _ in cs.index_breaks(kind):
                _accepted(b, way, kind, fn(t, x)[0], _expected(kind, None))
            xp = cs.record_near(t, kind.places()[place], True)
            for bit in (14, 15):                       # hapflag bits 14 - 15 are ignored (ecb.h), in a record that passes too
                _accepted(b, way, kind, cs.set_bit(t, xp, bit)[0], _expected(kind, None))


@pytest.mark.parametrize("name,way", COMBOS, ids=["%s-%s" % c for c in COMBOS])
@_a_hip_error_ends_the_session
def test_index_breaks_are_refused_where_the_table_says(name, way, monkeypatch):
    kind = cs.KINDS[name]
    b, kernel = _handle(kind, way, monkeypatch)
    with b:
        t = kind.base
        heads = cs.heads_of(t)
        for place in ("lane17+0", "short tile+1") + (("giant+0",) if kind.giant else ()):
            x = cs.record_near(t, kind.places()[place], True)
            for label, fn, _, field, value in cs.index_breaks(kind):
                if (field, value) == ("locus", 0xFFFFFFFF):             # (open: its LDS key is 0 -- see contract_streams.py)
                    continue
                at = _index_refused_at(way, field, value, place.startswith("giant"))
                _refused(b, way, fn(t, x)[0], INDEX_TEXT, at, cut=int(heads[heads <= x][-1]))
                _accepted(b, way, kind, t, _expected(kind, None))


@pytest.mark.parametrize("name", ["mid", "short"])
@_a_hip_error_ends_the_session
def test_a_stream_that_runs_past_the_hint(name, monkeypatch):
    """``ecb_hint_reads``: the base stream with one read fewer announced than it holds."""
    kind = cs.KINDS[name]
    th._force(monkeypatch, ("ECB_NO_PAR",))
    with ecb.EcBuilder(kind.n_loci, kind.n_haps, **SMALL) as b:
        for _ in range(2):
            b.hint_reads(kind.base["n_reads"] - 1)
            _refused(b, "device", kind.base, RUN_TEXT, "push")
            b.hint_reads(kind.base["n_reads"])
            assert _accepted(b, "device", kind, kind.base, _expected(kind, None)).startswith("ks_short::" if name == "short" else "ks_std::")


@pytest.mark.parametrize("way", ["device", "tiled"])
@_a_hip_error_ends_the_session
def test_a_push_that_does_not_continue_the_one_before(way, monkeypatch):
    """The base stream in two pushes cut at a head: the second one's read ids one too high (a jump over the cut) and two too low (a fall:
    its first record steps by -1); and so low that the stream would end below the reads already counted, which the host sees before it
    launches anything -- that refusal leaves the run as it was."""
    kind = cs.MID
    th._force(monkeypatch, ("ECB_NO_PAR",))
    t, exp = kind.base, _expected(kind, None)
    heads = cs.heads_of(t)
    c = int(heads[len(heads) // 2])
    part = lambda a, z, d=0: dict({k: t[k][a:z] for k in ("locus", "hapflag", "pos")}, read_id=((t["read_id"][a:z].astype(np.int64) + d) % cs.M32).astype(np.uint32))
    with ecb.EcBuilder(kind.n_loci, kind.n_haps, **SMALL) as b:
        for d in (1, -2):
            _push(b, way, part(0, c))
            with pytest.raises(ecb.EcbError) as e:
                _push(b, way, part(c, None, d))
            assert e.value.code == CONTRACT and RUN_TEXT in str(e.value)
            with pytest.raises(ecb.EcbError) as e:
                b.finalize()
            assert e.value.code == STATE and RUN_TEXT in str(e.value)
            b.reset()
        _push(b, way, part(0, c))
        with pytest.raises(ecb.EcbError) as e:
            _push(b, way, part(c, None, -int(t["read_id"][-1])))
        assert e.value.code == CONTRACT and "read_id went backwards across pushes" in str(e.value)
        _push(b, way, part(c, None))                                      # (not a refused run: the stream goes on)
        s = b.finalize()
        _check(b.export(), s, exp)
        assert np.array_equal(b.export_read_ec(), exp["read_ec"])


@pytest.mark.parametrize("name", ["mid", "long", "giant"])
@_a_hip_error_ends_the_session
def test_the_exactness_pass_refuses_a_broken_stream_and_the_run_goes_on(name, monkeypatch):
    """``ecb_verify_device`` / ``_tiled`` (k_stream<true>, the same phase (a)) over a broken stream of the same length: ECB_ERR_CONTRACT; the run
    is not refused; the clean stream then verifies with no read misplaced, and the handle finalizes to the oracle's result."""
    kind = cs.KINDS[name]
    th._force(monkeypatch, ("ECB_NO_PAR",))
    t, exp = kind.base, _expected(kind, None)
    d = _dev(t)[:3]
    tiles = ecb.tile_tuples(*d)
    with ecb.EcBuilder(kind.n_loci, kind.n_haps, **SMALL) as b:
        b.push_device(*d)
        want = b.verify_device(*d)
        assert want[0] == 0 and (want[1] > 0) == (kind.giant is not None)
        for i, (label, brk, which, x) in enumerate(c for c in cs.run_counter_cases(kind, every=False, refused_today=True) if c[2] is None):
            du = _dev(brk(t, x)[0])[:3]
            with pytest.raises(ecb.EcbError) as e:
                b.verify_device_tiled(ecb.tile_tuples(*du), cs.N) if i & 1 else b.verify_device(*du)
            assert e.value.code == CONTRACT and RUN_TEXT in str(e.value), label
            assert b.counters() == (exp["n_all"], exp["n_valid"], exp["n_reads"])
            assert (b.verify_device_tiled(tiles, cs.N) if i & 1 else b.verify_device(*d)) == want, label
        s = b.finalize()
        _check(b.export(), s, exp)


@_a_hip_error_ends_the_session
def test_a_shard_with_a_locus_out_of_range_is_refused_by_the_root(monkeypatch):
    """The multi-GPU path on one card: a shard whose stream has locus == n_loci in a passing record takes it (the stream kernel carries such a
    locus as data), its table is exported, and a root that merges or adopts it refuses at its finalize; so does ``ecb_merge``."""
    import torch
    kind = cs.MID
    th._force(monkeypatch, ("ECB_NO_PAR",))
    t = kind.base
    u, _ = cs.set_locus(t, cs.record_near(t, kind.places()["lane17+0"], True), kind.n_loci)
    d = _dev(u)[:3]
    with ecb.EcBuilder(kind.n_loci, kind.n_haps, **SMALL) as shard:
        shard.push_device(*d)
        ne, bound, _ = shard.table_sizes()
        ent = torch.zeros(4 * ne, dtype=torch.int64, device="cuda")
        prs = torch.zeros(bound, dtype=torch.int64, device="cuda")
        n_pairs = shard.table_export_parts_device(ent, prs, 0, 1)[1][-1]
        ctr = shard.counters()
    for take in ("merge", "adopt"):
        with ecb.EcBuilder(kind.n_loci, kind.n_haps, **SMALL) as root:
            (root.table_merge_device if take == "merge" else root.table_adopt_device)(ent, ne, prs, n_pairs)
            root.add_counters(*ctr)
            with pytest.raises(ecb.EcbError) as e:
                root.finalize()
            assert e.value.code == CONTRACT and INDEX_TEXT in str(e.value), take
    with ecb.EcBuilder(kind.n_loci, kind.n_haps, **SMALL) as shard, ecb.EcBuilder(kind.n_loci, kind.n_haps, **SMALL) as root:
        shard.push_device(*d)
        with pytest.raises(ecb.EcbError) as e:
            root.merge_from([shard])
        assert e.value.code == CONTRACT and INDEX_TEXT in str(e.value)
