"""bustools correct's rule restated in plain Python: a set, and a barcode's 3 x L single-base neighbours by string substitution on the
decoded sequence -- no bit is shifted or XOR-ed here, so this file cannot share the kernel's mistakes.  This file is the definition the
GPU tests compare with; ``tests/test_buscorrect.py`` holds it to a hand-written case."""
import numpy as np

from bus_checker import BASES, decode, encode

EXACT, CORRECTED, NO_CANDIDATE, AMBIGUOUS = 0, 1, 2, 3
_REC = [("bc", "<u8"), ("umi", "<u8"), ("ec", "<i4"), ("count", "<u4"), ("flags", "<u4"), ("pad", "<u4")]


def neighbours(seq):
    """The 3 x len(seq) sequences that differ from ``seq`` in exactly one base."""
    return [seq[:k] + c + seq[k + 1:] for k in range(len(seq)) for c in BASES if c != seq[k]]


def distance(a, b):
    """The number of bases in which two sequences of one length differ."""
    return sum(x != y for x, y in zip(a, b))


def outcome(barcode, bclen, white):
    """(status, barcode afterwards) of one barcode value against ``white``, a set of barcode values."""
    if barcode in white:
        return EXACT, barcode
    found = [v for v in (encode(s) for s in neighbours(decode(barcode, bclen))) if v in white]
    if len(found) == 1:
        return CORRECTED, found[0]
    return (AMBIGUOUS if found else NO_CANDIDATE), barcode


def correct(rec, bclen, whitelist):
    """What ``ecb_bus_correct`` returns: (status uint8 [n], the kept records uint8 [n_out, 32] in the file's order with the barcode of a
    corrected record replaced and nothing else touched, (exact, corrected, without a candidate, ambiguous))."""
    white = set(int(w) for w in whitelist)
    r = np.ascontiguousarray(rec).reshape(-1).copy().view(_REC)
    seen = {}
    status = np.zeros(len(r), dtype=np.uint8)
    for i, b in enumerate(r["bc"].tolist()):
        if b not in seen:
            seen[b] = outcome(b, bclen, white)
        status[i], new = seen[b]
        if status[i] == CORRECTED:
            r["bc"][i] = new
    kept = r[status <= CORRECTED].view(np.uint8).reshape(-1, 32)
    return status, kept, tuple(int((status == s).sum()) for s in (EXACT, CORRECTED, NO_CANDIDATE, AMBIGUOUS))
