"""A run that libecb refuses because the key arena ran out -- every place that answers ECB_ERR_TABLE_FULL for it -- and the handle afterwards.

Every case pushes one stream of ``refusal_streams.py`` twice: into a control handle with the usual small arena (2^24 pairs), whose result
must be the C oracle's bit for bit and which must have taken the path the case is about; and into a handle with an arena of 4 096 pairs,
which must answer -4 with a text that names the arena and its size.  The streams carry margins of four (``test_refusal_streams.py``
asserts them on the CPU), so neither outcome depends on how the waves pack their chunks.

After the refusal, on the same handle (``include/ecb.h``, under the error codes): every call but ``ecb_reset`` answers ECB_ERR_STATE, naming
the refusal, before it launches anything; ``ecb_reset`` succeeds; the recovery stream -- long keys again, within a quarter of the arena --
then gives A, N, the per-read EC ids and the counters of a fresh handle of the same configuration and of the oracle, bit for bit; and
once more, refusal, reset and recovery: a cursor left past a region's end and a wave's kept reservation do not survive a reset."""
import ctypes as C

import numpy as np
import pytest

from alntools_amd import ecb
from oracle import c_oracle
from oracle import ec_oracle as orc

import refusal_streams as rs
import test_gpu_thresholds as th
from test_gpu_parity import _check

pytestmark = pytest.mark.gpu

TABLE_FULL, STATE = -4, -6
SLOTS = 1 << 16                                                   # (no table growth in any case: at most 16 500 ECs)
CONTROL = dict(ec_capacity=SLOTS, arena_capacity=1 << 24)         # the arena of the poisoned-scratch tests' SMALL
TIGHT = dict(ec_capacity=SLOTS, arena_capacity=rs.ARENA)

_EXP = {}


def _expected(case, which):
    """The C oracle's result of a stream, with the EC of every read (the oracle's row that is the read's key), made once."""
    if (case.name, which) not in _EXP:
        t = getattr(case, which)
        exp = c_oracle.ec_from_tuples(t["read_id"], t["locus"], t["hapflag"], case.n_haps, threads=4)
        row = {tuple(zip(exp["indices"][a:z].tolist(), exp["data"][a:z].tolist())): e
               for e, (a, z) in enumerate(zip(exp["indptr"][:-1], exp["indptr"][1:]))}
        exp["read_ec"] = np.array([row[k] for k in rs.read_keys(t)], np.int32)
        exp["range"] = orc.ec_from_tuples(t["read_id"], t["locus"], t["hapflag"], case.n_loci, case.n_haps, pos=t["pos"])["range"]
        exp["read_ec"].setflags(write=False)
        _EXP[case.name, which] = exp
    return _EXP[case.name, which]


def _dev(t):
    import torch
    return [torch.from_numpy(t[k].view(np.int32)).cuda() for k in ("read_id", "locus", "hapflag", "pos")]


def _push(b, how, t, d):
    if how == "device":
        b.push_device(*(d if b.track_ranges else d[:3]))
    elif how == "tiled":
        b.push_device_tiled(ecb.tile_tuples(*d[:3]), len(t["read_id"]))
    else:
        b.push(t["read_id"], t["locus"], t["hapflag"], t["pos"] if b.track_ranges else None)


def _result(b):
    s = b.finalize()
    out = b.export()
    out.update(sizes=s, counters=b.counters(), read_ec=b.export_read_ec())
    if b.track_ranges:
        out["ranges"] = b.export_ranges()
    return out


def _same_as_the_oracle(got, exp):
    _check(got, got["sizes"], exp)
    assert got["counters"] == (exp["n_all"], exp["n_valid"], exp["n_reads"]) and got["sizes"]["n_reads"] == exp["n_reads"]
    assert np.array_equal(got["read_ec"], exp["read_ec"])
    if "ranges" in got:
        assert np.array_equal(got["ranges"], exp["range"])


def _same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(got[k], want[k]) if isinstance(want[k], np.ndarray) else got[k] == want[k], k


def _refused_then_every_call_says_so(b, refuse, again):
    """``refuse()`` is answered -4, naming the arena and its size; then finalize, the exports, table_sizes, the counters and a further push
    (``again``) are answered -6 with the refusal in the text, and so is the same call repeated."""
    with pytest.raises(ecb.EcbError) as e:
        refuse()
    first = (b._lib.ecb_last_error(b._h) or b"").decode()
    assert e.value.code == TABLE_FULL and "arena" in first and "%d pairs" % rs.ARENA in first, str(e.value)
    lib, none = b._lib, [None] * 6
    calls = [b.finalize, b.table_sizes, b.counters, again, lambda: b._chk(lib.ecb_export(b._h, *none)), lambda: b._chk(lib.ecb_export_device(b._h, *none)),
             lambda: b._chk(lib.ecb_export_read_ec(b._h, np.zeros(1 << 16, np.int32).ctypes.data_as(C.c_void_p))), refuse]
    for call in calls:
        with pytest.raises(ecb.EcbError) as e:
            call()
        assert e.value.code == STATE and first in str(e.value) and "(%d: " % TABLE_FULL in str(e.value) and "ecb_reset" in str(e.value), str(e.value)


def _two_rounds(make, refuse, case, how="device", recovery_hint=None):
    """refusal, reset, recovery == a fresh handle == the oracle; twice on one handle."""
    t = case.recovery
    d = _dev(t)
    exp = _expected(case, "recovery")

    def recover(b):
        if recovery_hint is not None:
            b.hint_reads(recovery_hint(exp["n_reads"]))
        _push(b, how, t, d)
        return _result(b)
    with make() as fresh:
        want = recover(fresh)
    _same_as_the_oracle(want, exp)
    with make() as b:
        for _ in range(2):
            _refused_then_every_call_says_so(b, lambda: refuse(b), lambda: _push(b, how, t, d))
            b.reset()
            assert (b._lib.ecb_last_error(b._h) or b"") == b""
            got = recover(b)
            _same(got, want)
            _same_as_the_oracle(got, exp)
            b.reset()


def _stream_case(case, how, monkeypatch, env, kernel, ranges=False, hinted=False, **tight):
    th._force(monkeypatch, env)
    t = case.refused
    d = _dev(t)
    exp = _expected(case, "refused")
    hint = (lambda n: n) if hinted else None

    def refuse(b):
        if hinted:
            b.hint_reads(exp["n_reads"])
        _push(b, how, t, d)
    with ecb.EcBuilder(case.n_loci, case.n_haps, track_ranges=ranges, **CONTROL) as c:
        refuse(c)
        c.counters()                                              # (a host push: the read it left open goes in)
        assert c.profile_kernel().startswith(kernel), c.profile_kernel()
        _same_as_the_oracle(_result(c), exp)
    _two_rounds(lambda: ecb.EcBuilder(case.n_loci, case.n_haps, track_ranges=ranges, **dict(TIGHT, **tight)), refuse, case, how, hint)


@pytest.mark.parametrize("how", ["device", "tiled", "host"])
def test_stream_kernel_founding_long_keys(how, monkeypatch):
    """ks_std: 600 distinct reads of 40 loci, through ecb_push_device, ecb_push_device_tiled and ecb_push in batches of 4 096 records."""
    _stream_case(rs.STD, how, monkeypatch, ("ECB_NO_PAR",), "ks_std::k_stream<false, false>", **({"max_batch_records": 4096} if how == "host" else {}))


def test_stream_kernel_with_ranges(monkeypatch):
    """The same stream with positions, through the compilation that tracks ranges; the ranges after the recovery are the recovery's alone."""
    _stream_case(rs.STD, "device", monkeypatch, None, "ks_std::k_stream<false, true>", ranges=True)


def test_short_read_kernel(monkeypatch):
    """ks_short (the reads hinted, six records each): one pair of every key goes to the arena, the waves' chunk reservations use it up."""
    _stream_case(rs.SHORT, "device", monkeypatch, None, "ks_short::", hinted=True)


def test_par_kernel(monkeypatch):
    """ks_par, forced, over the same keys."""
    _stream_case(rs.SHORT, "device", monkeypatch, ("ECB_FORCE_PAR",), "ks_par::")


def test_k_slow(monkeypatch):
    """Reads longer than a tile: k_slow founds their ECs (the exactness pass of the control handle sends them the same way)."""
    case = rs.SLOW
    with ecb.EcBuilder(case.n_loci, case.n_haps, **CONTROL) as c:
        for which in ("refused", "recovery"):
            d = _dev(getattr(case, which))[:3]
            c.push_device(*d)
            bad, n_long = c.verify_device(*d)
            assert bad == 0 and n_long > 0, (which, bad, n_long)
            c.reset()
    _stream_case(case, "device", monkeypatch, ("ECB_NO_PAR",), "ks_std::")


class _Table(object):
    """The table of a donor that holds ``rs.STD.refused``, as ranks exchange it."""

    def __init__(self):
        import torch
        case, t = rs.STD, rs.STD.refused
        with ecb.EcBuilder(case.n_loci, case.n_haps, **CONTROL) as donor:
            donor.push_device(*_dev(t)[:3])
            self.ne, bound, _ = donor.table_sizes()
            self.ent = torch.zeros(4 * self.ne, dtype=torch.int64, device="cuda")
            self.prs = torch.zeros(bound, dtype=torch.int64, device="cuda")
            self.np_ = donor.table_export_parts_device(self.ent, self.prs, 0, 1)[1][-1]
            self.ctr = donor.counters()
        assert self.np_ - rs.INL * self.ne >= 4 * rs.ARENA


@pytest.mark.parametrize("entry", ["merge", "adopt"])
def test_merge_and_adopt_of_a_table_of_long_keys(entry, monkeypatch):
    """k_merge founding the donor's long keys in a receiver with 4 096 pairs, and ``ecb_table_adopt_device``'s host check of the same table
    (decided before any kernel).  With room, both give the donor's result: the oracle's."""
    th._force(monkeypatch, None)
    case, T = rs.STD, _Table()
    exp = _expected(case, "refused")
    take = (lambda b: b.table_merge_device(T.ent, T.ne, T.prs, T.np_)) if entry == "merge" else (lambda b: b.table_adopt_device(T.ent, T.ne, T.prs, T.np_))
    with ecb.EcBuilder(case.n_loci, case.n_haps, **CONTROL) as c:
        take(c)
        c.add_counters(*T.ctr)
        s = c.finalize()
        _check(c.export(), s, exp)
        assert s["n_reads"] == exp["n_reads"]
    _two_rounds(lambda: ecb.EcBuilder(case.n_loci, case.n_haps, **TIGHT), take, case)


def test_reads_of_one_more_locus_than_a_tile_end_carries(monkeypatch):
    """``plan_stream`` sizes the deferred-read queue so that it cannot run out ("a read with more than CMAX loci takes more than CMAX
    records"): 300 reads of CMAX + 1 loci, each tile's last one ending on the tile's end, succeed and equal the oracle."""
    th._force(monkeypatch, ("ECB_NO_PAR",))
    t, T, H = rs.queue_stream()
    exp = c_oracle.ec_from_tuples(t["read_id"], t["locus"], t["hapflag"], H, threads=4)
    d = _dev(t)[:3]
    with ecb.EcBuilder(T, H, **CONTROL) as b:
        b.push_device(*d)
        assert b.profile_kernel().startswith("ks_std::")
        bad, n_long = b.verify_device(*d)
        print("reads deferred by the exactness pass:", n_long)
        assert bad == 0 and n_long > 0
        s = b.finalize()
        _check(b.export(), s, exp)
        assert s["n_reads"] == exp["n_reads"] == t["n_reads"]
