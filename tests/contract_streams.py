"""The streams of ``test_gpu_tuple_contract.py``: small streams that obey the tuple contract of ``include/ecb.h``, and named *breaks* of it, each
placed where the stream kernel's phase (a) (``k_stream.inc``) could lose sight of it: inside one lane's four records, across two lanes, across
the two halves of a tile, across tiles, across slices, in the stream's short last tile, inside a read longer than a tile.  Made on the CPU from
``alntools_amd/synth.py``'s counter-based random numbers; ``test_contract_streams.py`` proves on the CPU what each stream is.

A stream is a dict of the four tuple arrays plus ``n_reads``.  A break is a function ``(t, x) -> (t', words)``: ``t'`` differs from ``t`` in the
words ``words`` (a set of ``(field, index)``) at most, and breaks the rules in ``Break.rules`` -- those and no other.

Geometry (read from the kernel source as ``refusal_streams.py`` does): a tile holds ``WT`` = 512 records; lane ``l`` of the wave holds records
``4 l .. 4 l + 3`` of each 256-record half.  Every stream here is ``N = 4 WT + 100`` records long, which ``plan_stream`` cuts into slices of two
tiles: records ``[0, 2 WT)``, ``[2 WT, 4 WT)`` and the short last tile by itself.

THE OPEN HOLE these streams were built around, still open: phase (a) keeps ``step & 1`` per record and compares, per lane, the sum of its four
steps with the number of odd ones.  Steps that are even and cancel inside one lane's four records -- ``a, a + 2, a, a`` -- pass both, and a
passing record between them is keyed with a read index the pass's LDS table may have no room for.  ``old_phase_a`` restates that check; the
CPU test asserts that it accepts exactly the breaks for which ``Break.cancels`` holds.  Those cases stay out of the GPU tests
(``run_counter_cases(refused_today=True)``) until the kernel refuses them: checking every record's step was built and measured, and cost the
short-read stream 0.5 - 1 % of its kernel time, more than the project's margin (profiles/tuple_contract_ab.txt).  Locus 0xFFFFFFFF in a
passing record is the second open case (its LDS key is 0, an empty slot): kept on the CPU, not run on the GPU."""
import numpy as np

from oracle import ec_oracle as orc

import refusal_streams as rs

WT = rs.WT
N = 4 * WT + 100
PREFIX = 6                                     # leading records that do not pass the filter, read id 0xFFFFFFFF
PASS_PE, MATE_PE, UNMAPPED = 0x43, 0x83, 0x4   # paired + proper + read1: passes; read2: the mate, dropped; unmapped: dropped
PLAN_RULE = "waves = std::min<u64>(waves, (n + 2 * WT - 1) / (2 * WT));"
M32 = 1 << 32


def slice_edges(n):
    """``ecb.hip: plan_stream`` for a stream far smaller than the resident waves could share: ceil(n / 2 WT) slices of whole tiles."""
    waves = max(1, (n + 2 * WT - 1) // (2 * WT))
    chunk = ((n + waves - 1) // waves + WT - 1) // WT * WT
    return list(range(0, n, chunk))


# ---- places -----------------------------------------------------------------------------------------------------------------------------
# record index -> what is special about it.  Tile 1 (records WT .. 2 WT - 1) is the tile worked in: it has a tile before it and one behind.
PLACES = {}
for j in range(4):
    PLACES["lane0+%d" % j] = WT + j                       # (lane0+0: record 0 of a tile -- its step is taken from the tile before)
    PLACES["lane17+%d" % j] = WT + 4 * 17 + j
    PLACES["lane63+%d" % j] = WT + 252 + j                # (lane63+3: record 255, the last of the first half: 255 | 256)
    PLACES["half1+%d" % j] = WT + 256 + j                 # (half1+0: record 256 -- its step is taken from lane 63 of the first half)
    PLACES["last lane+%d" % j] = 2 * WT - 4 + j           # (+3: record 511, 511 | 512, and the slice edge behind it)
    PLACES["slice1+%d" % j] = 2 * WT + j                  # (slice1+0: the first record of a slice -- its step comes from another wave's tile)
    PLACES["short tile+%d" % j] = 4 * WT + 40 + j         # the stream's last tile, 100 records
EDGES = (WT, WT + 256, 2 * WT, 4 * WT)                    # a read that ends exactly here: tile, half, slice, the short tile's start


def in_one_lane(x, w):
    """Records x .. x + w (the changed ones and the first one behind them, where the counter returns) lie in one lane's group of four."""
    return x // 4 == (x + w) // 4


# ---- generator --------------------------------------------------------------------------------------------------------------------------
def _rnd(a, k, mod):
    return rs._rnd(a, k, mod)


class Kind(object):
    def __init__(self, name, paired, n_loci, n_haps, gap, salt, distinct=40, hinted=False, giant=None):
        self.name, self.paired, self.n_loci, self.n_haps, self.gap, self.salt = name, paired, n_loci, n_haps, gap, salt
        self.distinct, self.hinted, self.giant = distinct, hinted, giant
        self._made = {}

    def places(self):
        if self.giant is None:
            return dict(PLACES)
        g0 = self.giant[0]
        at = (g0 + 300) // 4 * 4
        return dict(PLACES, **{"giant+%d" % j: at + j for j in range(4)})

    def _heads(self, near_miss):
        gaps = self.gap[0] + _rnd(np.arange(N), self.salt, self.gap[1] - self.gap[0] + 1)
        heads = PREFIX + np.r_[0, np.cumsum(gaps)]
        heads = heads[heads < N]
        if self.giant is not None:                                    # one read of more than a tile's records
            heads = np.r_[heads[(heads < self.giant[0]) | (heads >= self.giant[1])], self.giant[0]]
        keep = np.ones(len(heads), bool)
        for x in self.places().values():                              # the base stream: no head on or next to a place (a break puts one there)
            keep &= (heads < x - 2) | (heads > x + 5)
        for x in EDGES:
            keep &= (heads != x)
        keep |= heads == PREFIX
        if self.giant is not None:
            keep |= heads == self.giant[0]
        heads = heads[keep]
        if near_miss is not None:                                     # a head on every place + near_miss, and (stream 0) a read that ends on every edge
            heads = np.r_[heads, [x for p, x in self.places().items() if p.endswith("+%d" % near_miss)], EDGES if near_miss == 0 else []]
        return np.unique(heads.astype(np.int64))

    def _make(self, near_miss):
        heads = self._heads(near_miss)
        i = np.arange(N, dtype=np.int64)
        r = np.searchsorted(heads, i, "right") - 1                    # (-1: the prefix)
        off = i - heads[np.maximum(r, 0)]
        inside = r >= 0
        length = np.diff(np.r_[heads, N])[np.maximum(r, 0)]
        valid = inside & ((((off & 1) == 0) | (length > WT)) if self.paired else True)          # (the giant read: every record passes)
        base = _rnd(np.maximum(r, 0), self.salt + 1, self.n_loci - N)
        step = np.where(length > WT, off, off // 2) if self.paired else off
        wrap = np.where(length > WT, N, self.distinct)                # (the giant read: every record on a locus of its own)
        loc = np.where(inside, base + step % wrap, 0)
        hap = np.where(inside, _rnd(base * 4096 + step, self.salt + 2, self.n_haps), 0)
        flag = np.where(~inside, UNMAPPED, np.where(valid, PASS_PE, MATE_PE) if self.paired else 0)
        t = dict(read_id=np.where(inside, r, 0xFFFFFFFF).astype(np.uint32), locus=loc.astype(np.uint32),
                 hapflag=((hap << 16) | flag).astype(np.uint32), pos=_rnd(i, self.salt + 3, 100000).astype(np.int32), n_reads=len(heads))
        for k in ("read_id", "locus", "hapflag", "pos"):
            t[k].setflags(write=False)
        return t

    def _get(self, which):
        if which not in self._made:
            self._made[which] = self._make(which)
        return self._made[which]

    @property
    def base(self):
        return self._get(None)

    @property
    def near_miss(self):
        """Four legal streams: number j has a head on every place ``name+j`` -- one head per lane group, so that the records around it belong
        to one read; in number 0 a read ends on every edge."""
        return [self._get(j) for j in range(4)]

    def stream(self, which):
        return self._get(which)


# mid: paired-end, about 16 reads of about 30 records per tile, every second record a mate that the filter drops
MID = Kind("mid", True, 30_000, 4, (24, 40), 1000)
# long: reads of 150 - 250 records on 40 loci: passes laid out for few reads, the layout in which a stray read index leaves the wave's table
LONG = Kind("long", False, 30_000, 4, (150, 250), 2000)
# short: 1 - 6 records per read, at most 8 haplotypes, the reads hinted: ks_short (reads next to a place are a few records longer)
SHORT = Kind("short", False, 30_000, 6, (1, 6), 3000, hinted=True)
# giant: mid with one read of 944 records, all of which pass, on 944 loci: more than a pass's table holds (WT + CMAX entries), so the stream
# kernel cannot but defer it to k_slow
GIANT = Kind("giant", True, 30_000, 4, (24, 40), 4000, giant=(2 * WT + 100, 4 * WT + 20))
KINDS = {k.name: k for k in (MID, LONG, SHORT, GIANT)}


def valid(t):
    return orc.tuples_valid(t["hapflag"])


def heads_of(t):
    rid = t["read_id"].astype(np.int64)
    return np.flatnonzero((rid - np.r_[0xFFFFFFFF, rid[:-1]]) % M32 == 1)


# ---- breaks -----------------------------------------------------------------------------------------------------------------------------
def _copy(t):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in t.items()}


def _add(t, x, deltas):
    """read_id[x + i] += deltas[i] (mod 2^32): the counter leaves its course at x and is back at x + len(deltas)."""
    u = _copy(t)
    for i, d in enumerate(deltas):
        u["read_id"][x + i] = (int(t["read_id"][x + i]) + d) % M32
    return u, {("read_id", x + i) for i in range(len(deltas))}


def _suffix(t, x, d, filtered=False):
    """read_id[x:] += d: the counter takes one wrong step at x and goes on from there (filtered: record x is made one that does not pass)."""
    u = _copy(t)
    u["read_id"][x:] = ((t["read_id"][x:].astype(np.int64) + d) % M32).astype(np.uint32)
    words = {("read_id", i) for i in range(x, len(t["read_id"]))}
    if filtered:
        u["hapflag"][x] |= UNMAPPED
        words.add(("hapflag", x))
    return u, words


class Break(object):
    """rules: what ``broken_rules`` must say of the broken stream.  width: records off course, the first of them record x + at (None: all
    from x on).  needs: what record x of the stream must be -- 'head', or 'inside' (not a head, the read goes on behind the break)."""

    def __init__(self, name, fn, rules, width=None, needs="inside", at=0):
        self.name, self.fn, self.rules, self.width, self.needs, self.at = name, fn, frozenset(rules), width, needs, at

    def __call__(self, t, x):
        return self.fn(t, x)

    def cancels(self, x):
        return self.width is not None and in_one_lane(x + self.at, self.width)


JUMPS, FALLS, FILTERED_STEP = "steps by more than one", "falls", "steps on a record that does not pass"
LOCUS, HAPLOTYPE, HIGH_BITS = "locus out of range", "haplotype out of range", "bits 24-31"

# the counter leaves its course and comes back: every step even (or 2^31 twice), their sum zero
CANCELLING = [
    Break("+2 -2", lambda t, x: _add(t, x, [2]), {JUMPS, FALLS}, 1),
    Break("+2 0 -2", lambda t, x: _add(t, x, [2, 2]), {JUMPS, FALLS}, 2),
    Break("+2^31 -2^31", lambda t, x: _add(t, x, [1 << 31]), {JUMPS}, 1),
    Break("+4 -2 -2", lambda t, x: _add(t, x, [4, 2]), {JUMPS, FALLS}, 2),
]
# (x a head of the near-miss stream, a legal +1 on a passing record; the record behind it goes +2 and back: a, a+1, a+3, a+1)
AFTER_A_HEAD = Break("+1 +2 -2", lambda t, x: _add(t, x + 1, [2]), {JUMPS, FALLS}, 1, needs="head", at=1)
# one wrong step, and on from there
ONE_WAY = [
    Break("+2 on a passing record", lambda t, x: _suffix(t, x, 1), {JUMPS}, needs="head"),
    Break("+1 on a filtered record", lambda t, x: _suffix(t, x, 1, filtered=True), {FILTERED_STEP}),
    Break("-1", lambda t, x: _suffix(t, x, -1), {FALLS}),
]
AFTER_A_HEAD_31 = Break("+1 +2^31 -2^31", lambda t, x: _add(t, x + 1, [1 << 31]), {JUMPS}, 1, needs="head", at=1)
RUN_COUNTER = CANCELLING + [AFTER_A_HEAD, AFTER_A_HEAD_31] + ONE_WAY


def run_counter_cases(kind, every=True, refused_today=False):
    """-> [(label, break, which stream (None: base; j: near miss j), x)].  every: each break at each place; else "+2 -2" at each place and
    every other break at a quarter of the places, a different quarter each.  refused_today: without the cases of THE OPEN HOLE -- those whose
    steps cancel within one lane's four records, which phase (a) lets through and which must therefore not be run on a GPU."""
    out = []
    for i, (place, x) in enumerate(sorted(kind.places().items(), key=lambda kv: kv[1])):
        for k, b in enumerate(RUN_COUNTER):
            if refused_today and b.cancels(x):
                continue
            if every or b is CANCELLING[0] or (i + k) % 4 == 0:
                out.append(("%s at %s" % (b.name, place), b, int(place[-1]) if b.needs == "head" else None, x))
    return out


def set_locus(t, x, v):
    u = _copy(t)
    u["locus"][x] = v
    return u, {("locus", x)}


def set_hap(t, x, v):
    u = _copy(t)
    u["hapflag"][x] = (int(t["hapflag"][x]) & ~0x00FF0000) | (v << 16)
    return u, {("hapflag", x)}


def set_bit(t, x, b):
    u = _copy(t)
    u["hapflag"][x] |= np.uint32(1 << b)
    return u, {("hapflag", x)}


def index_breaks(kind):
    """-> [(name, fn(t, x), rule, field, value)]: an index of a record out of range (a break when the record passes, nothing when it does not)."""
    out = []
    for v in (kind.n_loci, (1 << 25) - 2, (1 << 26) - 3, (1 << 26) - 2, 0xFFFFFFFF):
        out.append(("locus %d" % v, (lambda t, x, v=v: set_locus(t, x, v)), LOCUS, "locus", v))
    for v in (kind.n_haps, 8, 31, 32, 255):
        out.append(("haplotype %d" % v, (lambda t, x, v=v: set_hap(t, x, v)), HAPLOTYPE, "hap", v))
    for b in (24, 31):
        out.append(("bit %d" % b, (lambda t, x, b=b: set_bit(t, x, b)), HIGH_BITS, "bit", b))
    return out


def record_near(t, x, passing):
    """The first record at or behind x that passes the filter (or does not) and is no head."""
    v, h = valid(t), set(heads_of(t).tolist())
    while bool(v[x]) != passing or x in h:
        x += 1
    return x


def a_filtered_record(t, x):
    """A record that does not pass, at or behind x if the stream has one there (paired-end: a mate), else one of the prefix."""
    v = valid(t)
    later = np.flatnonzero(~v[x:])
    return x + int(later[0]) if len(later) else 2


# ---- what a stream breaks ---------------------------------------------------------------------------------------------------------------
def broken_rules(t, n_loci, n_haps):
    """The rules of the tuple contract that ``t`` breaks, by name (the empty set: ``obeys_contract``).  Steps are taken modulo 2^32, as the
    counter is a u32 that starts at 0xFFFFFFFF: 2 .. 2^31 is a jump, anything above a fall."""
    rid, hf = t["read_id"].astype(np.int64), t["hapflag"].astype(np.int64)
    v = valid(t)
    step = (rid - np.r_[0xFFFFFFFF, rid[:-1]]) % M32
    out = set()
    if np.any((step >= 2) & (step <= 1 << 31)):
        out.add(JUMPS)
    if np.any(step > 1 << 31):
        out.add(FALLS)
    if np.any((step == 1) & ~v):
        out.add(FILTERED_STEP)
    if np.any(t["locus"][v] >= n_loci):
        out.add(LOCUS)
    if np.any(((hf[v] >> 16) & 0xFF) >= n_haps):
        out.add(HAPLOTYPE)
    if np.any((hf[v] >> 24) != 0):
        out.add(HIGH_BITS)
    return out


def old_phase_a(t):
    """The check phase (a) made before it looked at every step: per lane and half tile, D = the counter's difference over the lane's four
    records, H = the number of odd steps among them -- steps looked at only at the two positions (even, odd) at which some lane of the half
    holds a record that passes -- and whether an odd step sits on a record that does not pass.  -> (D, H, odd step on a filtered record)."""
    n = len(t["read_id"])
    pad = (-n) % WT
    rid = np.r_[t["read_id"].astype(np.int64), np.full(pad, t["read_id"][-1], np.int64)]      # (load_tile: past the end, the last id again)
    ok = np.r_[valid(t), np.zeros(pad, bool)]
    step = (rid - np.r_[0xFFFFFFFF, rid[:-1]]) % M32
    half = np.arange(len(rid)) // 256
    par = np.arange(len(rid)) & 1
    seen = np.zeros((len(rid) // 256, 2), bool)
    np.logical_or.at(seen, (half[ok], par[ok]), True)
    odd = ((step & 1) == 1) & seen[half, par]
    D = step.reshape(-1, 4).sum(axis=1) % M32
    H = odd.reshape(-1, 4).sum(axis=1)
    return D, H, bool(np.any(odd & ~ok))


def differing_words(t, u):
    return {(k, int(i)) for k in ("read_id", "locus", "hapflag", "pos") for i in np.flatnonzero(t[k] != u[k])}
