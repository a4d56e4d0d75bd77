"""salmon2ec restated with numpy, independently of the reference and of libecb, and a seeded writer of salmon directories of any size.

``expected`` gives what ``alntools salmon2ec`` writes: transcripts and haplotypes numbered by first appearance in the header (``-t``
names appended), lengths truncated toward zero, A[e, t] = the OR of 2^h over the line's targets of transcript t, N = the ECs with a
non-zero count.  ``parse_section`` restates the EC-section rules of ``ecb_salmon_ecs`` line by line and raises :class:`Refusal` with the
lowest offending line and reason code."""
import gzip
import os

import numpy as np

R_BYTE, R_EMPTY, R_BIG, R_FEW, R_K, R_TARGET, R_REPEAT, R_COUNT = range(1, 9)


class Refusal(ValueError):
    def __init__(self, line, reason):
        ValueError.__init__(self, "EC line %d: reason %d" % (line, reason))
        self.line, self.reason = line, reason


def _line_reason(line, n_targets):
    """The reason code of one EC line (without its line end), or 0, and its target ids."""
    if any(c not in b"0123456789\t" for c in line):
        return R_BYTE, None
    fields = line.split(b"\t")
    if any(f == b"" for f in fields):
        return R_EMPTY, None
    vals = [int(f) for f in fields]
    if any(v >= 2 ** 31 for v in vals):
        return R_BIG, None
    if len(vals) < 2:
        return R_FEW, None
    if vals[0] != len(vals) - 2:
        return R_K, None
    tids = vals[1:-1]
    if any(t >= n_targets for t in tids):
        return R_TARGET, None
    if len(set(tids)) != len(tids):
        return R_REPEAT, None
    return 0, (tids, vals[-1])


def parse_section(section, n_ecs, n_targets):
    """The EC section's bytes -> (per line the list of target ids, counts); :class:`Refusal` at the lowest offending line."""
    lines = section.split(b"\n")
    if lines and lines[-1] == b"":                     # (a final line end; a missing one is accepted)
        lines.pop()
        last_open = False
    else:
        last_open = True                               # (its \r, if any, is not before a line end)
    rows, counts = [], []
    for i, raw in enumerate(lines):
        ended = i + 1 < len(lines) or not last_open
        line = raw[:-1] if ended and raw.endswith(b"\r") else raw
        r, got = _line_reason(line, n_targets)
        if r:
            raise Refusal(i, r)
        rows.append(got[0])
        counts.append(got[1])
    if len(lines) != n_ecs:
        raise Refusal(min(len(lines), n_ecs), R_COUNT)
    return rows, np.array(counts, dtype=np.int64)


def number_names(names, extra=()):
    tid, hid = {}, {}
    col = np.array([tid.setdefault(n.split("_")[0], len(tid)) for n in names], dtype=np.int64)
    hap = np.array([hid.setdefault(n.split("_")[1], len(hid)) for n in names], dtype=np.int64)
    for t in extra:
        tid.setdefault(t, len(tid))
    return list(tid), list(hid), col, hap


def csr_from_targets(ec_ptr, ec_tid, col, hap, n_loci):
    """CSR A from the EC -> target-id lists (ec_ptr / ec_tid, ids distinct within an EC): a lexsort by (row, column), OR per run."""
    E = len(ec_ptr) - 1
    row = np.repeat(np.arange(E, dtype=np.int64), np.diff(ec_ptr))
    c, bits = col[ec_tid], np.left_shift(1, hap[ec_tid]).astype(np.int64)
    key = row * n_loci + c
    order = np.argsort(key, kind="stable")
    key, bits = key[order], bits[order]
    head = np.ones(len(key), dtype=bool)
    head[1:] = key[1:] != key[:-1]
    starts = np.flatnonzero(head)
    data = np.bitwise_or.reduceat(bits, starts) if len(starts) else np.zeros(0, dtype=np.int64)
    ukey = key[starts]
    indptr = np.searchsorted(ukey // max(n_loci, 1), np.arange(E + 1), side="left") if len(ukey) else np.zeros(E + 1, dtype=np.int64)
    return indptr, ukey % max(n_loci, 1), data


def expected(names, eff_lengths, ec_ptr, ec_tid, counts, extra=()):
    """(hname, lname, lengths, indptrA, indicesA, dataA, indptrN, indicesN, dataN) of the .bin."""
    lname, hname, col, hap = number_names(names, extra)
    lengths = np.zeros((len(lname), len(hname)), dtype=np.int64)
    lengths[col, hap] = np.trunc(np.asarray(eff_lengths, dtype=np.float64)).astype(np.int64)
    ip, ix, da = csr_from_targets(np.asarray(ec_ptr), np.asarray(ec_tid, dtype=np.int64), col, hap, len(lname))
    counts = np.asarray(counts, dtype=np.int64)
    nz = np.flatnonzero(counts)
    return hname, lname, lengths, ip, ix, da, np.array([0, len(nz)]), nz, counts[nz]


def expected_from_dir(d, target_file=None):
    """``expected`` of a salmon directory on disk (header, quant.sf and EC section parsed here; refusals raise)."""
    p = os.path.join(d, "aux_info", "eq_classes.txt")
    data = open(p, "rb").read() if os.path.exists(p) else gzip.decompress(open(p + ".gz", "rb").read())
    head = data.split(b"\n", 2)
    T, E = int(head[0]), int(head[1])
    rest = head[2].split(b"\n", T)
    names = [n.decode().rstrip() for n in rest[:T]]
    section = rest[T] if len(rest) > T else b""
    eff = {}
    with open(os.path.join(d, "quant.sf")) as fh:
        fh.readline()
        for line in fh:
            item = line.rstrip().split("\t")
            eff[item[0]] = float(item[2])
    rows, counts = parse_section(section, E, T)
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    tid = np.array([t for r in rows for t in r], dtype=np.int64)
    extra = []
    if target_file:
        extra = [str(t) for t in np.loadtxt(target_file, dtype=str, delimiter="\t", usecols=(0,), ndmin=1)]
    return expected(names, [eff[n] for n in names], ptr, tid, counts, extra)


# ---- writer -------------------------------------------------------------------------------------------------------------------------
def format_ints(tok, sep):
    """bytes of the non-negative integers ``tok``, each followed by its byte in ``sep`` (vectorized: no per-line Python)."""
    tok = np.asarray(tok, dtype=np.int64)
    nd = np.ones(len(tok), dtype=np.int64)
    for d in range(1, 19):
        nd += tok >= 10 ** d
    start = np.concatenate([[0], np.cumsum(nd + 1)[:-1]]) if len(tok) else np.zeros(0, dtype=np.int64)
    out = np.empty(int((nd + 1).sum()), dtype=np.uint8)
    for d in range(int(nd.max()) if len(tok) else 0):
        m = nd > d
        out[start[m] + nd[m] - 1 - d] = 48 + (tok[m] // 10 ** d) % 10
    out[start + nd] = sep
    return out.tobytes()


def ec_section(ec_ptr, ec_tid, counts, crlf=False):
    """The EC section of the ECs ``ec_ptr`` / ``ec_tid`` (target ids per EC) with ``counts``: ``k t_1 .. t_k count`` per line."""
    ec_ptr = np.asarray(ec_ptr, dtype=np.int64)
    E = len(ec_ptr) - 1
    k = np.diff(ec_ptr)
    n_tok = k + 2
    tstart = np.concatenate([[0], np.cumsum(n_tok)[:-1]])
    tok = np.empty(int(n_tok.sum()), dtype=np.int64)
    tok[tstart] = k
    tok[tstart + n_tok - 1] = counts
    inner = np.ones(len(tok), dtype=bool)
    inner[tstart] = False
    inner[tstart + n_tok - 1] = False
    tok[inner] = ec_tid
    sep = np.full(len(tok), 9, dtype=np.uint8)
    sep[tstart + n_tok - 1] = 10
    text = format_ints(tok, sep) if E else b""
    return text.replace(b"\n", b"\r\n") if crlf else text


def random_ecs(rng, n_targets, n_ecs, mean_k=4.0, long_every=0, long_k=(100, 900), zero_frac=0.05, empty_frac=0.02):
    """ECs of distinct target ids: mostly short, one in ``long_every`` long; some counts 0, some ECs without targets."""
    k = rng.poisson(mean_k - 1, size=n_ecs) + 1
    if long_every:
        big = rng.random(n_ecs) < 1.0 / long_every
        k[big] = rng.integers(long_k[0], long_k[1] + 1, size=int(big.sum()))
    k[rng.random(n_ecs) < empty_frac] = 0
    k = np.minimum(k, n_targets)
    ptr = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
    # distinct ids within an EC: a random offset plus a sorted sample of gaps, shuffled
    tid = np.empty(int(ptr[-1]), dtype=np.int64)
    for e in np.flatnonzero(k > 0):
        tid[ptr[e]:ptr[e + 1]] = rng.choice(n_targets, size=int(k[e]), replace=False)
    counts = rng.integers(1, 1000, size=n_ecs)
    counts[rng.random(n_ecs) < zero_frac] = 0
    return ptr, tid, counts


def random_ecs_fast(rng, n_targets, n_ecs, mean_k=11.0):
    """Many ECs quickly (config-3 size): k ~ 1 + Poisson(mean_k - 1), ids = a random start plus strictly increasing gaps (mod T:
    distinct while k * max_gap < T), shuffled within the EC by a random rotation."""
    k = np.minimum(rng.poisson(mean_k - 1, size=n_ecs) + 1, 200)
    ptr = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
    n = int(ptr[-1])
    row = np.repeat(np.arange(n_ecs), k)
    gaps = rng.integers(1, 64, size=n)
    gaps[ptr[:-1]] = rng.integers(0, n_targets, size=n_ecs)
    tid = np.cumsum(gaps)
    tid -= np.repeat(tid[ptr[:-1]] - gaps[ptr[:-1]], k)
    tid %= n_targets
    rot = rng.integers(0, 2, size=n_ecs).astype(bool)          # half the ECs written in descending order
    flip = np.repeat(rot, k)
    pos = np.arange(n) - ptr[row]
    src = np.where(flip, ptr[row] + (k[row] - 1 - pos), np.arange(n))
    tid = tid[src]
    counts = rng.integers(1, 100, size=n_ecs)
    counts[rng.random(n_ecs) < 0.02] = 0
    return ptr, tid, counts


def target_names(n_tx, haps, rng=None):
    """T = n_tx * len(haps) names ``TX<i>_<hap>``; with ``rng`` the order is shuffled (first appearance then decides the numbering)."""
    names = ["TX%06d_%s" % (t, h) for t in range(n_tx) for h in haps]
    if rng is not None:
        names = [names[i] for i in rng.permutation(len(names))]
    return names


def write_salmon_dir(d, names, eff_lengths, section, n_ecs, gz=False, header_extra=b""):
    """aux_info/eq_classes.txt (or .txt.gz) and quant.sf."""
    os.makedirs(os.path.join(d, "aux_info"), exist_ok=True)
    head = ("%d\n%d\n" % (len(names), n_ecs)).encode() + "".join(n + "\n" for n in names).encode() + header_extra
    p = os.path.join(d, "aux_info", "eq_classes.txt")
    if gz:
        with gzip.open(p + ".gz", "wb", compresslevel=1) as fh:
            fh.write(head + section)
    else:
        with open(p, "wb") as fh:
            fh.write(head)
            fh.write(section)
    with open(os.path.join(d, "quant.sf"), "w") as fh:
        fh.write("Name\tLength\tEffectiveLength\tTPM\tNumReads\n")
        for n, e in zip(names, eff_lengths):
            fh.write("%s\t%d\t%s\t1.0\t1.0\n" % (n, int(e) + 50, repr(float(e))))
