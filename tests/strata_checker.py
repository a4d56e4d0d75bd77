"""The best-stratum rule, as a plain loop over reads: what ``ecb_best_strata`` must give, byte for byte.  No numpy tricks and no bit
arithmetic beyond the filter.  ``tests/test_best_strata.py`` holds it to a hand-written dozen of records."""
import numpy as np

DROP_BITS = 0x4 | 0x4000


def passes(hf):
    """``rec_valid`` of ``csrc/ecb.hip`` (``tuples.record_valid`` with the two host bits 12 and 13)."""
    if hf & 0x4:
        return False
    if hf & 0x1:
        if (hf & 0x80) or not (hf & 0x2) or (hf & 0x1000) or (hf & 0x2000):
            return False
    return True


def breach(read_id, hapflag):
    """``(record, reason)`` of the lowest record that breaks the contract, or None."""
    for i in range(1, len(read_id)):
        d = (int(read_id[i]) - int(read_id[i - 1])) % (1 << 32)
        if d == 0:
            continue
        if d == 1:
            if not passes(int(hapflag[i])):
                return i, "read_id steps on a record that does not pass the filter"
        elif d < (1 << 31):
            return i, "read_id steps by more than 1"
        else:
            return i, "read_id falls"
    return None


def best_strata(read_id, hapflag, score, lowest=True):
    """-> ``(out_read_id uint32, out_hapflag uint32, (passing, kept, dropped, reads whose first passing record was dropped))``."""
    n = len(read_id)
    out_id = [int(x) for x in read_id]
    out_hf = [int(x) for x in hapflag]
    n_pass = n_kept = n_drop = n_first = 0
    start = 0
    while start < n:
        end = start
        while end < n and int(read_id[end]) == int(read_id[start]):
            end += 1
        members = [i for i in range(start, end) if passes(int(hapflag[i]))]
        if members:
            scores = [int(score[i]) for i in members]
            best = min(scores) if lowest else max(scores)
            kept = [i for i in members if int(score[i]) == best]
            for i in members:
                if int(score[i]) != best:
                    out_hf[i] = out_hf[i] | DROP_BITS
            for i in range(start, kept[0]):
                out_id[i] = (int(read_id[i]) - 1) % (1 << 32)
            n_pass += len(members)
            n_kept += len(kept)
            n_drop += len(members) - len(kept)
            if kept[0] != members[0]:
                n_first += 1
        start = end
    return np.array(out_id, dtype=np.uint32), np.array(out_hf, dtype=np.uint32), (n_pass, n_kept, n_drop, n_first)


def kept_mask(read_id, hapflag, score, lowest=True):
    """True for every record the rule does not drop (kept and non-passing records alike)."""
    _, out_hf, _ = best_strata(read_id, hapflag, score, lowest)
    return np.array([int(o) == int(h) for o, h in zip(out_hf, hapflag)], dtype=bool)
