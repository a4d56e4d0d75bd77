"""The tuple contract of ``include/ecb.h`` as a predicate on a whole stream: what ``refusal_streams.py`` and ``contract_streams.py`` hold
their inputs to."""
import numpy as np

from oracle import ec_oracle as orc


def obeys_contract(t, n_loci, n_haps):
    """The tuple contract of ``include/ecb.h``: the run counter starts at 0xFFFFFFFF or 0, never falls, steps by one and only on a valid
    record; loci and haplotypes of valid records in range; no bit outside flag, host bits and haplotype."""
    rid, hf = t["read_id"].astype(np.int64), t["hapflag"].astype(np.int64)
    v = orc.tuples_valid(t["hapflag"])
    prev = np.r_[-1, np.where(rid == 0xFFFFFFFF, -1, rid)[:-1]]
    cur = np.where(rid == 0xFFFFFFFF, -1, rid)
    step = cur - prev
    return bool(len(rid) and np.all((step == 0) | ((step == 1) & v)) and np.all(t["locus"][v] < n_loci)
                and np.all(((hf[v] >> 16) & 0xFF) < n_haps) and np.all((hf & ~0x00FF3FFF) == 0)
                and all(t[k].dtype == np.uint32 for k in ("read_id", "locus", "hapflag")) and t["pos"].dtype == np.int32)
