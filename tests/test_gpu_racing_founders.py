"""The EC table with many waves founding the same ECs at once.  ``test_gpu_flush_rounds.py`` and ``test_gpu_hash_collisions.py`` cover
what can happen inside one wave; here the waves of one launch race each other.  ``racing_streams.py`` lays every stream out on the slices
of the launch (``plan_stream`` cuts a batch of S x 1024 records, S <= 256, into S slices of two tiles, all resident at once), and every
slice founds the same ECs in the same order (or its neighbours' a pass earlier or later, or the other key of a slot or of a hash): a lost
claim, a slot that carries a hash and no ``n1`` yet, a key whose pairs are still being stored are then the common case, not an accident
of a hot EC.  Which of these outcomes the streams reach is measured with the ``-DECB_TIMING`` build's race counters, outside the suite:
``profiles/racing_founders.txt``.

Every family runs through ``ks_std``, ``ks_par`` and ``ks_short`` (forced, and reported by ``profile_kernel``), three times in one test --
a run takes well under a millisecond and the interleavings differ from run to run -- as one device push and as whole tiles; all three
runs must equal ``oracle.c_oracle`` on the whole stream bit for bit (CSR A, N, the three counters), with as many ECs as the family has
keys and as many occupied slots as ECs (no key sits in two slots); the exactness pass must then find no read in a wrong EC.  A bounded
spin that gives up (``SPIN_MAX``, the 64 settle rounds) surfaces as ``EcbError``: a finding to read the code for.

``k_merge`` takes all tables of a call in one launch: eight shards that pushed the same reads export the same keys in the same order
into a root whose table maps a hash to the same slot -- an aligned race of eight -- merged in one call, by key ranges and adopted, and
through ``ecb_merge``."""
import numpy as np
import pytest

from alntools_amd import ecb
from oracle import c_oracle

import racing_streams as rs
from test_gpu_flush_rounds import _check
from test_gpu_hash_collisions import _assert_collide, _device_hashes, _rows_of
from test_gpu_thresholds import COMPILATIONS, KNOBS, _every_push

pytestmark = pytest.mark.gpu

T, H = rs.T, rs.H
RUNS = 3
THREE = ("std", "par", "short")                # ks_std, ks_par, ks_short (COMPILATIONS' fourth is ks_std again, with the reads hinted)
FAMILIES = [f for f in sorted(rs.FAMILIES) if f != "ranges"]


def _force(monkeypatch, env):
    for k in KNOBS + ("ECB_ROUNDS", "ECB_MIN_TILES"):           # (the slices are 1024 records whatever the two say; the defaults all the same)
        monkeypatch.delenv(k, raising=False)
    for k in env or ():
        monkeypatch.setenv(k, "1")


def _dev(t, keys=("read_id", "locus", "hapflag")):
    import torch
    return [torch.from_numpy(t[k].view(np.int32).copy()).cuda() for k in keys]


def _colliding_rows_apart(b, exp, info):
    """As ``test_gpu_hash_collisions._witness``: the two ECs of a committed collision have equal exported hashes and different rows."""
    if info.get("colliding"):
        pairs = [tuple((np.array(k[0]), np.array(k[1])) for k in p) for p in info["colliding"]]
        _assert_collide(_device_hashes(b), _rows_of(exp["indptr"], exp["indices"], exp["data"]), pairs)


def _one_run(b, push, kernel, hint, exp, info):
    if hint:
        b.hint_reads(hint)
    push(b)
    assert b.profile_kernel().startswith(kernel), b.profile_kernel()
    slots = b.table_sizes()[0]
    s = b.finalize()
    _check(b.export(), s, exp)
    assert s["n_ecs"] == info["n_ecs"] == slots, (s["n_ecs"], info["n_ecs"], slots)       # no EC twice, no key in two slots
    return s


def _race(name, comp, monkeypatch, pos=False):
    t, info, exp = rs.family(name)
    env, hinted, kernel = COMPILATIONS[comp]
    _force(monkeypatch, env)
    rs.assert_aligned(t)
    d = _dev(t, ("read_id", "locus", "hapflag") + (("pos",) if pos else ()))
    n = len(t["read_id"])
    tiles = None if pos else ecb.tile_tuples(*d)
    hint = t["n_reads"] if hinted else 0
    small = name in rs.SMALL_TABLE
    kw = dict(ec_capacity=rs.CAP_SMALL) if small else {}
    if pos:
        kw["track_ranges"] = True
        kernel = "ks_std::k_stream<false, true>"
        mn, mx = rs.range_minmax(t)
    pushes = [lambda b: b.push_device(*d), (lambda b: b.push_device(*d)) if pos else (lambda b: b.push_device_tiled(tiles, n)), lambda b: b.push_device(*d)]
    b = ecb.EcBuilder(T, H, **kw)
    try:
        for run in range(RUNS):
            if run and small:                   # (a handle that has grown keeps its table over a reset: the small table is a new handle's)
                b.close()
                b = ecb.EcBuilder(T, H, **kw)
            elif run:
                b.reset()
            _one_run(b, pushes[run], kernel, hint, exp, info)
            if run == 0:
                _colliding_rows_apart(b, exp, info)
            if pos:
                gmn, gmx = b.export_range_minmax()
                assert np.array_equal(gmn.reshape(-1), mn) and np.array_equal(gmx.reshape(-1), mx), run
        b.reset()
        if hint:
            b.hint_reads(hint)
        b.push_device(*d)
        assert b.verify_device(*d[:3]) == (0, info.get("n_long", 0))
    finally:
        b.close()


@pytest.mark.parametrize("comp", THREE)
@pytest.mark.parametrize("name", FAMILIES)
def test_every_wave_of_the_launch_founds_the_same_ecs(name, comp, monkeypatch):
    """Three runs per compilation, every one == the C oracle; ``verify_device`` reports 0 misplaced reads and exactly the reads of the
    giants families (one per slice) on the long path.  same_slot and growth start every run on a new table of 1024 slots (growth parks,
    grows and resumes with 16 waves per block still racing); same_hash's colliding ECs have equal exported hashes and different rows."""
    _race(name, comp, monkeypatch)


def test_racing_founders_with_the_range_update_fused_in(monkeypatch):
    """``track_ranges=True`` (``ks_std::k_stream<false, true>``, whatever is forced): same_order with a position per record that depends on
    the slice.  The founder's sentinel and the other racers' minima and maxima meet on the same words: ``export_range_minmax`` == numpy's
    minimum and maximum per (locus, haplotype), (INT_MAX, INT_MIN) where no record points."""
    _race("ranges", "std", monkeypatch, pos=True)


@pytest.mark.parametrize("name", [f for f in FAMILIES if f not in rs.SMALL_TABLE and f != "same_order_256"])
def test_the_racing_streams_through_every_push(name, monkeypatch):
    """The default table will do: ``test_gpu_thresholds._every_push`` -- every compilation as one device push and as tiles, the host push in an
    odd batch size (which breaks the alignment, and is harmless), the exactness pass with the family's long reads."""
    t, info, exp = rs.family(name)
    _force(monkeypatch, None)
    n_long = info.get("n_long", 0)
    _every_push({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in t.items()}, T, H, exp, monkeypatch, batches=(4097,), n_long=(n_long, n_long))


# ---- k_merge ------------------------------------------------------------------------------------------------------------------------------
_SHARDS = {}


def _merge_case():
    if not _SHARDS:
        t, info = rs.merge_shard()
        whole = rs.concatenated(t)
        _SHARDS.update(t=t, info=info, exp=c_oracle.ec_from_tuples(whole["read_id"], whole["locus"], whole["hapflag"], H, threads=4))
    return _SHARDS["t"], _SHARDS["info"], _SHARDS["exp"]


def _pushed_shards(t):
    d = _dev(t)
    out = []
    for _ in range(rs.N_SHARDS):
        b = ecb.EcBuilder(T, H)
        b.push_device(*d)
        out.append(b)
    return out


def _check_root(b, exp, info):
    """(``ecb_merge`` leaves its root finalized: the occupied slots are counted where the handle still holds a table to count)"""
    slots = b.table_sizes()[0] if b.sizes is None else info["n_ecs"]
    s = b.sizes or b.finalize()
    _check(b.export(), s, exp)
    assert s["n_ecs"] == info["n_ecs"] == slots, (s["n_ecs"], info["n_ecs"], slots)
    _colliding_rows_apart(b, exp, info)


def test_eight_tables_of_the_same_keys_in_one_merge_launch():
    """Eight shards that pushed the same ~3 000 short keys, 28 long keys and 24 pairs of colliding keys: the same table layout and the same
    export order, so the eight tables of one ``table_merge_batch_device`` call bring every key at the same moment to the same slot of a
    root of the shards' (default) capacity.  (a) merged whole in one call, three times; (b) cut into two key ranges, each merged in one
    call on a handle of its own and the parts adopted by ``table_adopt_batch_device``; (c) ``merge_from``.  Each == the C oracle on the eight
    streams concatenated with their read bases."""
    import torch
    from alntools_amd import dist as ecdist
    dev = torch.device("cuda:0")
    t, info, exp = _merge_case()
    shards = _pushed_shards(t)
    whole, parts, totals, base = [], [], [0, 0, 0], 0
    for b in shards:
        eng = ecdist.GpuEngine(b, dev)
        ne, npairs, nreads = b.table_sizes()
        assert ne == info["n_ecs"] and nreads == t["n_reads"]
        whole.append(eng.table_export(base) + (ne, npairs))
        parts.append(eng.table_export_parts(base, 2))
        totals = [x + y for x, y in zip(totals, b.counters())]
        base += nreads
    # (c) first: ecb_merge takes the shards as they are, pushed and not finalized
    with ecb.EcBuilder(T, H) as root:
        root.merge_from(shards)
        _check_root(root, exp, info)
    for b in shards:
        b.close()
    # (a)
    for _ in range(RUNS):
        with ecb.EcBuilder(T, H) as root:
            ecdist.GpuEngine(root, dev).table_merge_many([(ent, ne, prs, npairs) for ent, prs, ne, npairs in whole])
            root.add_counters(*totals)
            _check_root(root, exp, info)
    # (b)
    adopted = []
    for q in range(2):
        with ecb.EcBuilder(T, H) as part:
            eng = ecdist.GpuEngine(part, dev)
            eng.table_merge_many([(ent[eo[q] * 4:eo[q + 1] * 4], eo[q + 1] - eo[q], prs[po[q]:po[q + 1]], po[q + 1] - po[q]) for ent, prs, eo, po in parts])
            pe_n, pp_n, _ = part.table_sizes()
            adopted.append(eng.table_export(0) + (pe_n, pp_n))
    assert sum(a[2] for a in adopted) == info["n_ecs"]
    with ecb.EcBuilder(T, H) as root:
        ecdist.GpuEngine(root, dev).table_adopt_many([(pe, pe_n, pp, pp_n) for pe, pp, pe_n, pp_n in adopted])
        root.add_counters(*totals)
        _check_root(root, exp, info)
