"""Every device entry point of libecb on caller memory as a caller has it: offset, guarded views of one larger tensor
(``tests/caller_views.py``: every array at a chosen residue of its address modulo 16, 256 guard bytes of its own on both sides, inputs
copied, outputs pre-filled over their documented room).  A fresh ``torch`` allocation -- what every other GPU test hands in -- is 256-byte
aligned and nobody reads what follows it; so the element-by-element branches behind the kernels' 16-byte paths (``k_gm_check``,
``k_gm_scatter``, ``sel_load4``, ``k_sel_gather_a``'s four-at-once store, ``sl_load``) ran for the last, ragged thread of a call only,
and a write one element past an output went unseen.

After every call here: the return code, the result bit for bit against the checker the entry's own tests use (ecquant: within its derived
bound, and bit for bit the same call on aligned tensors), and ``Slab.check()`` empty -- no guard byte touched on either side of any array,
no input changed.  Part 1: the entry points that take a device, at the shapes DESIGN.md section 4 lists (nnz just above two workgroups
of the four-per-thread passes, every residue of nnz modulo 4, one row longer than a workgroup, stored masks of 0 where the entry takes
them), each array placement its own case.  Part 2: the entry points that take a handle -- the one alignment rule ecb.h states (the
streams of ecb_push_device* / ecb_verify_device*: refused, the run as it was) and everything else the handle reads from and writes into
caller memory at natural alignment off 16 bytes."""
import ctypes as C

import numpy as np
import pytest

from alntools_amd import bin_utils, ecb

import bundle_checker as bchk
import counts_checker
import ec_merge_checker as chk
import gt_checker
import quant_checker as qchk
import salmon_checker as schk
import select_checker
import test_gpu_ecbundle as tb
import test_gpu_multisample as tm
import test_gpu_poisoned_scratch as tps
from caller_views import MARGIN, Slab
from test_gpu_parity import _check

pytestmark = pytest.mark.gpu

ARG, CONTRACT = -1, -5
T, H, S = 1200, 8, 11          # (T: a row longer than one workgroup's 1 024 entries needs that many columns)
LONG_ROW, LONG_AT, BAD_ROW = 1030, 77, 100
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _P(t):
    return ecb._dev_ptr(t)


# ---- the matrices -------------------------------------------------------------------------------------------------------------------------
def _matrix(k, zeros, n_haps=H):
    """E = 230 rows of 0 .. 9 entries and one of 1 030 (so ``k_sel_gather_a`` meets four entries of one row and four of several),
    nnz(A) = 2 052 + k -- just above two workgroups of 1 024 entries, every residue modulo 4 -- and nnz(N) just above 2 048 over 11
    samples, one of them with two reads only; ``zeros``: some stored masks and some stored counts of 0."""
    def make():
        rng = np.random.default_rng(100 + k + 10 * zeros + n_haps)
        lens = rng.integers(0, 10, size=230)
        lens[LONG_AT] = LONG_ROW
        short = [e for e in range(230) if e != LONG_AT]
        j = 0
        while lens.sum() != 2052 + k:
            e = short[j % len(short)]
            j += 1
            if lens.sum() < 2052 + k and lens[e] < 9:
                lens[e] += 1
            elif lens.sum() > 2052 + k and lens[e] > 0:
                lens[e] -= 1
        rows = []
        for n in lens:
            masks = rng.integers(1, 1 << n_haps, size=int(n), dtype=np.int64)
            if n == 1 and rng.random() < 0.7:
                masks[0] = 1 << int(rng.integers(0, n_haps))             # (rows of one set bit: ecselect's class "unique")
            if zeros:
                masks[rng.random(int(n)) < 0.05] = 0
            rows.append((np.sort(rng.choice(T, size=int(n), replace=False)), masks))
        E = len(rows)
        m = tb._m(rows, n_haps, T, sname=["s%d" % s for s in range(S)])
        ip, ix, dx = [0], [], []
        for s in range(S):
            if s == 3:                                                   # (two reads in all: below any threshold from 3 on)
                listed, cnt = np.array([5, LONG_AT + 1]), np.array([1, 1])
            else:
                listed = np.flatnonzero(rng.random(E) < 0.95)
                if s == 0:
                    listed = np.union1d(listed, [LONG_AT])               # (the long row is counted: it stays wherever its class does)
                cnt = rng.integers(1, 40, size=len(listed))
                if zeros and s != 0:
                    cnt[rng.random(len(listed)) < 0.03] = 0
            ix.append(listed); dx.append(cnt); ip.append(ip[-1] + len(listed))
        m.indptrN, m.indicesN, m.dataN = (np.asarray(x, dtype=np.int32) for x in (ip, np.concatenate(ix), np.concatenate(dx)))
        assert len(m.indicesA) == 2052 + k and 2048 < len(m.indicesN) < 2048 + 256 and int(np.diff(m.indptrA).max()) == LONG_ROW
        assert bool((m.dataA == 0).any()) == bool(zeros) and bool((m.dataN == 0).any()) == bool(zeros)
        return m
    return _cached(("matrix", k, zeros, n_haps), make)


def _falling(ip):
    """Row pointers that fall once, in the middle (the malformed input of every CSR taker's own refusal test)."""
    bad = np.array(ip).copy()
    bad[BAD_ROW], bad[BAD_ROW + 1] = ip[BAD_ROW + 1] + 1, ip[BAD_ROW]
    return bad


def _csr_ins(m, n=True):
    ins = [("ip", m.indptrA, np.int32), ("ix", m.indicesA, np.int32), ("da", m.dataA, np.int32)]
    return ins + ([("pn", m.indptrN, np.int32), ("xn", m.indicesN, np.int32), ("dn", m.dataN, np.int32)] if n else [])


class Case(object):
    """One entry point on one input: ``ins`` [(name, array, dtype)], ``outs`` [(name, shape, dtype)], ``call(v)`` -> (rc, scalars) on the
    placed views ``v``, ``verify(out, scalars)`` on the outputs read back, ``bad`` = (name of an input, its malformed version, code)."""

    def __init__(self, ins, outs, call, verify, bad=None):
        self.ins, self.outs, self.call, self.verify, self.bad = ins, outs, call, verify, bad

    names = property(lambda s: [i[0] for i in s.ins] + [o[0] for o in s.outs])


def _same(got, want, what):
    assert np.array_equal(np.asarray(got, dtype=np.int64), np.asarray(want, dtype=np.int64)), what


# ---- part 1: one Case per entry point ----------------------------------------------------------------------------------------------------
def _conv_matrix(key):
    return _matrix(0, 0, 31) if key == "h31" else _matrix(key, 0)


def _hapcsc_of(key):
    def make():
        m = _conv_matrix(key)
        nh = m.num_haplotypes
        row = np.repeat(np.arange(m.num_reads), np.diff(m.indptrA))
        k, h = np.nonzero((m.dataA.astype(np.int64)[:, None] >> np.arange(nh)[None, :]) & 1)
        return tps._hapcsc(m.num_reads, T, nh, row[k], m.indicesA[k].astype(np.int64), h)
    return _cached(("hapcsc", key), make)


def case_csr_to_hapcsc_count(key):
    m = _conv_matrix(key)
    lib, nh = ecb.load(), m.num_haplotypes

    def call(v):
        tot = C.c_uint64(0xDEAD)
        rc = lib.ecb_csr_to_hapcsc_device(0, m.num_reads, T, nh, _P(v["ip"]), _P(v["ix"]), _P(v["da"]), None, None, C.byref(tot))
        return rc, tot.value

    def verify(out, tot):
        assert tot == int(np.unpackbits(m.dataA.view(np.uint8)).sum())
    return Case(_csr_ins(m, n=False), [], call, verify)


def case_csr_to_hapcsc(key):
    m = _conv_matrix(key)
    lib, nh = ecb.load(), m.num_haplotypes
    csr, (cp, ci) = _hapcsc_of(key)

    def call(v):
        tot = C.c_uint64(0xDEAD)
        rc = lib.ecb_csr_to_hapcsc_device(0, m.num_reads, T, nh, _P(v["ip"]), _P(v["ix"]), _P(v["da"]), _P(v["cp"]), _P(v["ci"]), C.byref(tot))
        return rc, tot.value

    def verify(out, tot):
        assert tot == len(ci)
        _same(out["cp"], cp, "cp"); _same(out["ci"], ci, "ci")
    return Case(_csr_ins(m, n=False), [("cp", (nh, T + 1), np.int32), ("ci", (len(ci),), np.int32)], call, verify,
                bad=("ip", _falling(m.indptrA), CONTRACT))


def case_hapcsc_to_csr(key):
    m = _conv_matrix(key)
    lib, nh = ecb.load(), m.num_haplotypes
    csr, (cp, ci) = _hapcsc_of(key)
    total = len(ci)

    def call(v):
        nnz = C.c_uint64(0xDEAD)
        rc = lib.ecb_hapcsc_to_csr_device(0, m.num_reads, T, nh, _P(v["cp"]), _P(v["ci"]), total, _P(v["ip"]), _P(v["ix"]), _P(v["da"]), C.byref(nnz))
        return rc, nnz.value

    def verify(out, nnz):
        assert nnz == len(csr[1])
        _same(out["ip"], csr[0], "ip"); _same(out["ix"][:nnz], csr[1], "ix"); _same(out["da"][:nnz], csr[2], "da")
    bad = cp.copy()
    bad[0, 10], bad[0, 11] = cp[0, 11] + 1, cp[0, 10]                    # (a falling column pointer: this entry's malformed input)
    return Case([("cp", cp, np.int32), ("ci", ci, np.int32)],
                [("ip", (m.num_reads + 1,), np.int32), ("ix", (total,), np.int32), ("da", (total,), np.int32)], call, verify, bad=("cp", bad, CONTRACT))


def case_apply_mask(key):
    m = _matrix(key, 1)
    lib, nnz = ecb.load(), len(m.indicesA)
    mask = np.random.default_rng(key).integers(0, 1 << H, size=T, dtype=np.int64).astype(np.uint32)
    exp = gt_checker.mask_csr(m.indptrA, m.indicesA, m.dataA, mask)

    def call(v):
        kept = C.c_uint64(0xDEAD)
        rc = lib.ecb_apply_mask_device(0, m.num_reads, T, H, nnz, _P(v["ip"]), _P(v["ix"]), _P(v["da"]), _P(v["mask"]), _P(v["oip"]), _P(v["oix"]),
                                       _P(v["oda"]), C.byref(kept))
        return rc, kept.value

    def verify(out, kept):
        assert kept == len(exp[1]) < nnz
        _same(out["oip"], exp[0], "indptr"); _same(out["oix"][:kept], exp[1], "indices"); _same(out["oda"][:kept], exp[2], "data")
    return Case(_csr_ins(m, n=False) + [("mask", mask, np.uint32)],
                [("oip", (m.num_reads + 1,), np.int32), ("oix", (nnz,), np.int32), ("oda", (nnz,), np.int32)], call, verify,
                bad=("ip", _falling(m.indptrA), CONTRACT))


def case_count_alignments(key):
    m = _matrix(key, 1)
    lib = ecb.load()
    sample = None if key % 2 == 0 else 2
    exp = counts_checker.count(m.indptrA, m.indicesA, m.dataA, T, H, m.indptrN, m.indicesN, m.dataN, sample=sample)

    def call(v):
        rc = lib.ecb_count_alignments_device(0, m.num_reads, T, H, len(m.indicesA), _P(v["ip"]), _P(v["ix"]), _P(v["da"]), S, len(m.indicesN),
                                             _P(v["pn"]), _P(v["xn"]), _P(v["dn"]), -1 if sample is None else sample, _P(v["aln"]), _P(v["uniq"]),
                                             _P(v["lu"]))
        return rc, None

    def verify(out, _):
        for name, e in zip(("aln", "uniq", "lu"), exp):
            _same(out[name], e, name)
    return Case(_csr_ins(m), [("aln", (H, T), np.int64), ("uniq", (H, T), np.int64), ("lu", (T,), np.int64)], call, verify,
                bad=("ip", _falling(m.indptrA), CONTRACT))


def case_select(key):
    m = _matrix(key, 1)
    lib, nnz, nnz_n = ecb.load(), len(m.indicesA), len(m.indicesN)
    row_class = select_checker.CLASSES[key]                              # every row, unique, locus-unique, multi
    keep = np.ones(S, dtype=bool)
    keep[[1, 8]] = False
    mincount = 3                                                          # (sample 3 counts two reads: it goes)
    exp, stay, rows = select_checker.select_flags(m, row_class, keep, mincount)
    assert not stay[3] and stay.sum() == S - 3 and rows.any() and bool(rows[LONG_AT]) == (row_class in (None, "multi"))

    def call(v):
        sizes = (C.c_uint64 * 4)(*[0xDEAD] * 4)
        rc = lib.ecb_select_device(0, m.num_reads, T, H, S, nnz, _P(v["ip"]), _P(v["ix"]), _P(v["da"]), nnz_n, _P(v["pn"]), _P(v["xn"]), _P(v["dn"]),
                                   ecb.ROW_CLASSES[row_class], _P(v["skeep"]), mincount, _P(v["oip"]), _P(v["oix"]), _P(v["oda"]), _P(v["opn"]),
                                   _P(v["oxn"]), _P(v["odn"]), _P(v["okeep"]), sizes)
        return rc, [int(x) for x in sizes]

    def verify(out, sizes):
        E2, a2, S2, n2 = sizes
        assert (E2, a2, S2, n2) == (exp.num_reads, len(exp.indicesA), exp.num_samples, len(exp.indicesN))
        _same(out["oip"][:E2 + 1], exp.indptrA, "indptrA"); _same(out["oix"][:a2], exp.indicesA, "indicesA"); _same(out["oda"][:a2], exp.dataA, "dataA")
        _same(out["opn"][:S2 + 1], exp.indptrN, "indptrN"); _same(out["oxn"][:n2], exp.indicesN, "indicesN"); _same(out["odn"][:n2], exp.dataN, "dataN")
        _same(out["okeep"] != 0, stay, "kept samples")
    return Case(_csr_ins(m) + [("skeep", keep.astype(np.uint8), np.uint8)],
                [("oip", (m.num_reads + 1,), np.int32), ("oix", (nnz,), np.int32), ("oda", (nnz,), np.int32), ("opn", (S + 1,), np.int32),
                 ("oxn", (nnz_n,), np.int32), ("odn", (nnz_n,), np.int32), ("okeep", (S,), np.uint8)], call, verify,
                bad=("ip", _falling(m.indptrA), CONTRACT))


def case_bundle(key):
    m = _matrix(key, 0)
    lib, nnz, nnz_n = ecb.load(), len(m.indicesA), len(m.indicesN)
    groups = tb._grouping("mixed", np.random.default_rng(key), T)
    mp, mi = bchk.group_csr(T, groups)
    exp = _cached(("bundle", key), lambda: bchk.bundle(m, tb._names(len(groups)), groups))
    cap = min(int(np.diff(mp.astype(np.int64))[m.indicesA].sum()), m.num_reads * len(groups))      # (ecb_bundle.h: the caller's bound X)

    def call(v):
        sizes = (C.c_uint64 * 3)(*[0xDEAD] * 3)
        rc = lib.ecb_bundle_device(0, m.num_reads, T, H, S, len(groups), nnz, _P(v["ip"]), _P(v["ix"]), _P(v["da"]), nnz_n, _P(v["pn"]), _P(v["xn"]),
                                   _P(v["dn"]), len(mi), _P(v["mp"]), _P(v["mi"]), cap, _P(v["oip"]), _P(v["oix"]), _P(v["oda"]), _P(v["opn"]),
                                   _P(v["oxn"]), _P(v["odn"]), sizes)
        return rc, [int(x) for x in sizes]
    return Case(_csr_ins(m) + [("mp", mp, np.uint32), ("mi", mi, np.uint32)],
                [("oip", (m.num_reads + 1,), np.int32), ("oix", (cap,), np.int32), ("oda", (cap,), np.int32), ("opn", (S + 1,), np.int32),
                 ("oxn", (nnz_n,), np.int32), ("odn", (nnz_n,), np.int32)], call, lambda out, sizes: _verify_bin(out, sizes, exp),
                bad=("ip", _falling(m.indptrA), CONTRACT))


def _verify_bin(out, sizes, exp):
    """The six arrays of a combined or bundled .bin against the checker's ``ECMatrices``."""
    E2, a2, n2 = sizes
    assert (E2, a2, n2) == (exp.num_reads, len(exp.indicesA), len(exp.indicesN))
    _same(out["oip"][:E2 + 1], exp.indptrA, "indptrA"); _same(out["oix"][:a2], exp.indicesA, "indicesA"); _same(out["oda"][:a2], exp.dataA, "dataA")
    _same(out["opn"], exp.indptrN, "indptrN"); _same(out["oxn"][:n2], exp.indicesN, "indicesN"); _same(out["odn"][:n2], exp.dataN, "dataN")


def case_combine(key):
    """Two parts: the matrix, and a smaller one over the same targets in another order (a ``target_map``) whose samples overlap the
    first part's (both carry a ``sample_map``)."""
    m0 = _matrix(key, 0)

    def make():
        rng = np.random.default_rng(7 + key)
        small = chk.random_bin(rng, 150, m0.lname, m0.hname, ["s2", "x1", "s9", "x2"], max_row=50)
        small.lengths = m0.lengths
        m1 = chk.permute_targets(small, rng)
        return m1, bin_utils.plan_merge([m0, m1]), chk.merge([m0, m1])
    m1, plan, exp = _cached(("combine", key), make)
    lib = ecb.load()
    assert np.array_equal(plan.target_maps[0], np.arange(T)) and not np.array_equal(plan.target_maps[1], np.arange(T))
    ins = []
    for k, (m, tmap, smap) in enumerate(zip((m0, m1), (None, plan.target_maps[1]), plan.sample_maps)):
        ins += [("p%d_%s" % (k, n), a, dt) for n, a, dt in _csr_ins(m)]
        ins += [("p%d_tm" % k, tmap, np.uint32)] if tmap is not None else []
        ins += [("p%d_sm" % k, smap, np.uint32)]
    R, NP, NZ = m0.num_reads + m1.num_reads, len(m0.indicesA) + len(m1.indicesA), len(m0.indicesN) + len(m1.indicesN)
    n_samples = len(plan.sname)

    def call(v):
        cp = (ecb.CombinePart * 2)()
        for k, m in enumerate((m0, m1)):
            c = cp[k]
            c.struct_size, c.n_ecs, c.n_samples, c.n_loci = C.sizeof(ecb.CombinePart), m.num_reads, m.num_samples, T
            c.nnz_a, c.nnz_n = len(m.indicesA), len(m.indicesN)
            for field, name in (("indptr_a", "ip"), ("indices_a", "ix"), ("data_a", "da"), ("indptr_n", "pn"), ("indices_n", "xn"), ("data_n", "dn"),
                                ("target_map", "tm"), ("sample_map", "sm")):
                t = v.get("p%d_%s" % (k, name))
                setattr(c, field, None if t is None else t.data_ptr())
        sizes = (C.c_uint64 * 3)(*[0xDEAD] * 3)
        rc = lib.ecb_combine_device(0, 2, cp, T, H, n_samples, _P(v["oip"]), _P(v["oix"]), _P(v["oda"]), _P(v["opn"]), _P(v["oxn"]), _P(v["odn"]), sizes)
        return rc, [int(x) for x in sizes]
    return Case(ins, [("oip", (R + 1,), np.int32), ("oix", (NP,), np.int32), ("oda", (NP,), np.int32), ("opn", (n_samples + 1,), np.int32),
                      ("oxn", (NZ,), np.int32), ("odn", (NZ,), np.int32)], call, lambda out, sizes: _verify_bin(out, sizes, exp),
                bad=("p0_ip", _falling(m0.indptrA), CONTRACT))


def _quantify(m, v, scale="scale"):
    it, dl, ex, cv = C.c_uint32(77), C.c_double(7.25), C.c_int64(77), C.c_uint32(77)
    rc = ecb.load().ecb_quantify_device(0, m.num_reads, T, H, len(m.indicesA), _P(v["ip"]), _P(v["ix"]), _P(v["da"]), S, len(m.indicesN), _P(v["pn"]),
                                        _P(v["xn"]), _P(v["dn"]), -1, _P(v[scale]), _P(v["theta_in"]), 1, 0.0, _P(v["theta"]), C.byref(it),
                                        C.byref(dl), C.byref(ex), C.byref(cv))
    return rc, (it.value, dl.value, ex.value, cv.value)


def case_quantify(key):
    """One step (``max_iters=1``, ``tol=0``) from a given theta with a scale: within the step's derived bound of the checker's, and bit for
    bit what the same call gives on tensors of their own (determinism is part of ecquant's contract)."""
    import torch
    m = _matrix(key, 1)
    rng = np.random.default_rng(20 + key)
    theta_in = rng.random((H, T)) * 10 + 0.01
    theta_in[:, m.indicesA[m.indptrA[5]:m.indptrA[6]]] = 0.0             # (a row whose targets all have theta = 0)
    scale = 1.0 / rng.integers(1, 3000, size=(H, T))
    p = qchk.Problem.of(m)
    ref, explained = qchk.step(p, theta_in, scale)

    def aligned():
        v = {n: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda() for n, a, dt in _csr_ins(m)}
        v.update(scale=torch.from_numpy(scale).cuda(), theta_in=torch.from_numpy(theta_in).cuda(),
                 theta=torch.full((H, T), 7.25, dtype=torch.float64, device="cuda"))
        assert all(t.data_ptr() % 16 == 0 for t in v.values())
        rc, scal = _quantify(m, v)
        assert rc == 0
        torch.cuda.synchronize()
        return v["theta"].cpu().numpy().tobytes(), scal
    plain, plain_scal = _cached(("quant_aligned", key), aligned)

    def verify(out, scal):
        qchk.agree(out["theta"], ref, p.tolerance())
        assert scal[0] == 1 and scal[2] == explained and scal[3] == 0
        assert out["theta"].tobytes() == plain and scal == plain_scal
    bad = scale.copy()
    bad[1, T // 2] = np.nan
    return Case(_csr_ins(m) + [("scale", scale, np.float64), ("theta_in", theta_in, np.float64)], [("theta", (H, T), np.float64)],
                lambda v: _quantify(m, v), verify, bad=("scale", bad, CONTRACT))


SALMON_PADS = (15, 16, 17, 4095, 4096, 4097)


def _salmon_input(key):
    """(text, n_ecs, col, hap, n_loci, n_haps, expected five arrays): the text of test_gpu_salmon2ec.py::
    test_long_fields_and_line_ends_at_every_offset for a pad, or one random section of 5 000 ECs."""
    def make():
        if key == "random":
            rng = np.random.default_rng(52)
            names = schk.target_names(150, ["h%d" % h for h in range(4)], rng)
            ptr, tid, counts = schk.random_ecs(rng, len(names), 5000, mean_k=6.0, long_every=50, long_k=(50, 400))
            lname, hname, col, hap = schk.number_names(names)
            exp = schk.expected(names, rng.uniform(0, 5000, size=len(names)), ptr, tid, counts)
            return schk.ec_section(ptr, tid, counts), 5000, col, hap, len(lname), len(hname), (exp[3], exp[4], exp[5], exp[7], exp[8])
        text = b"1\t" + b"0" * key + b"3\t" + b"0" * (key // 2) + b"42\n2\t9\t8\t1"
        return text, 2, np.arange(10) // 2, np.arange(10) % 2, 5, 2, ([0, 1, 2], [1, 4], [2, 3], [0, 1], [42, 1])
    return _cached(("salmon", key), make)


def case_salmon_ecs(key):
    text, E, col, hap, n_loci, n_haps, exp = _salmon_input(key)
    lib = ecb.load()
    raw = np.frombuffer(text, dtype=np.uint8)
    cap = int((raw == 9).sum()) - E

    def call(v, text_name="text"):
        sizes = (C.c_uint64 * 2)(*[0xDEAD] * 2)
        rc = lib.ecb_salmon_ecs_device(0, _P(v[text_name]), len(raw), E, len(col), _P(v["tcol"]), _P(v["thap"]), n_loci, n_haps, cap, _P(v["oip"]),
                                       _P(v["oix"]), _P(v["oda"]), _P(v["onx"]), _P(v["ond"]), sizes)
        return rc, [int(x) for x in sizes]

    def verify(out, sizes):
        nnz, nnz_n = sizes
        assert (nnz, nnz_n) == (len(exp[1]), len(exp[3]))
        for name, n, e in (("oip", E + 1, exp[0]), ("oix", nnz, exp[1]), ("oda", nnz, exp[2]), ("onx", nnz_n, exp[3]), ("ond", nnz_n, exp[4])):
            _same(out[name][:n], e, name)
    bad = raw.copy()
    at = len(raw) // 2
    while not 48 <= bad[at] <= 57:
        at += 1
    bad[at] = ord("x")                                                    # (a byte that is no digit, tab or line end: reason 1)
    return Case([("text", raw, np.uint8), ("tcol", col, np.uint32), ("thap", hap, np.uint32)],
                [("oip", (E + 1,), np.int32), ("oix", (cap,), np.int32), ("oda", (cap,), np.int32), ("onx", (E,), np.int32), ("ond", (E,), np.int32)],
                call, verify, bad=("text", bad, CONTRACT))


CSR = ["ip", "ix", "da"]
CSR_N = CSR + ["pn", "xn", "dn"]
BIN_OUT = ["oip", "oix", "oda", "opn", "oxn", "odn"]
#: entry point -> (its Case, its inputs' keys, its arrays in the order they are placed)
ENTRIES = {
    "csr_to_hapcsc_count": (case_csr_to_hapcsc_count, (0, 1, 2, 3, "h31"), CSR),
    "csr_to_hapcsc": (case_csr_to_hapcsc, (0, 1, 2, 3, "h31"), CSR + ["cp", "ci"]),
    "hapcsc_to_csr": (case_hapcsc_to_csr, (0, 1, 2, 3, "h31"), ["cp", "ci"] + CSR),
    "apply_mask": (case_apply_mask, (0, 1, 2, 3), CSR + ["mask", "oip", "oix", "oda"]),
    "count_alignments": (case_count_alignments, (0, 1, 2, 3), CSR_N + ["aln", "uniq", "lu"]),
    "select": (case_select, (0, 1, 2, 3), CSR_N + ["skeep"] + BIN_OUT + ["okeep"]),
    "bundle": (case_bundle, (0, 1, 2, 3), CSR_N + ["mp", "mi"] + BIN_OUT),
    "combine": (case_combine, (0, 1, 2, 3), ["p0_" + n for n in CSR_N] + ["p0_sm"] + ["p1_" + n for n in CSR_N] + ["p1_tm", "p1_sm"] + BIN_OUT),
    "quantify": (case_quantify, (0, 1, 2, 3), CSR_N + ["scale", "theta_in", "theta"]),
    "salmon_ecs": (case_salmon_ecs, SALMON_PADS + ("random",), ["text", "tcol", "thap", "oip", "oix", "oda", "onx", "ond"]),
}


def _case(entry, key):
    return _cached(("case", entry, key), lambda: ENTRIES[entry][0](key))


def _residue(placement, name, itemsize):
    """Where array ``name`` goes under ``placement``: ``control`` (every array on 16 bytes), ``all4`` / ``all8`` / ``all12`` (4-byte
    arrays there, 8-byte arrays at 8, bytes at 1 / 7 / 15), ``one:<name>`` (that array at 4 -- 8 for 8-byte elements -- the rest at 0)."""
    if placement == "control":
        return 0
    if placement.startswith("one:"):
        return 0 if placement[4:] != name else 8 if itemsize == 8 else 4
    r = int(placement[3:])
    return {4: r, 8: 8, 1: {4: 1, 8: 7, 12: 15}[r]}[itemsize]


def _place(case, placement, extra=()):
    ins = list(case.ins) + list(extra)
    room = sum(np.asarray(a).size * np.dtype(dt).itemsize for _, a, dt in ins) + sum(int(np.prod(sh)) * np.dtype(dt).itemsize for _, sh, dt in case.outs)
    slab = Slab("cuda", nbytes=room + (len(ins) + len(case.outs) + 1) * (2 * MARGIN + 16))
    v = {}
    for name, a, dt in ins:
        v[name] = slab.place(name, a, dt, _residue(placement, name.split("~")[0], np.dtype(dt).itemsize), "in")
    for name, shape, dt in case.outs:
        v[name] = slab.place(name, shape, dt, _residue(placement, name, np.dtype(dt).itemsize), "out")
    return slab, v


def _outputs(case, slab, host):
    return {name: slab.room(name, host).view(dt).reshape(shape) for name, shape, dt in case.outs}


def _good_call(case, slab, v):
    import torch
    rc, scalars = case.call(v)
    torch.cuda.synchronize()
    assert rc == 0, (rc, ecb.load().ecb_last_error(None))
    host = slab.host()
    case.verify(_outputs(case, slab, host), scalars)
    assert slab.check(host) == []


PLACED = [(e, k, p) for e, (_, keys, names) in ENTRIES.items() for k in keys
          for p in ["control", "all4", "all8", "all12"] + ["one:" + n for n in names]]


@pytest.mark.parametrize("entry,key,placement", PLACED, ids=["%s-%s-%s" % c for c in PLACED])
def test_entry_points_that_take_a_device(entry, key, placement):
    """``control``: every array on a 16-byte boundary of the slab -- the vector paths, under the guard check.  ``all4`` / ``all8`` /
    ``all12``: no array on one -- the element-by-element paths in every thread.  ``one:<name>``: one array off, the others on: an alignment
    test that forgot one of the pointers it has to cover would take the vector path with that pointer off 16 bytes.  What that does on
    gfx950 is not known here (every such test was read and covers its pointers), so these cases promise no more
    than this: a forgotten pointer shows as a wrong result or a touched guard byte, if it shows at all."""
    case = _case(entry, key)
    assert case.names == ENTRIES[entry][2]
    slab, v = _place(case, placement)
    if placement != "control":
        assert any(t.data_ptr() % 16 for t in v.values())
    _good_call(case, slab, v)


@pytest.mark.parametrize("entry", [e for e in ENTRIES if e != "csr_to_hapcsc_count"])
def test_a_refused_call_on_offset_views_leaves_the_outputs_and_the_guards_alone(entry):
    """The entry's own malformed input (a falling row or column pointer, a bad byte, a NaN in ``scale``) with every array at residue 4:
    the documented code, the whole room of every output still 0x5C, every guard byte intact, and the good call right behind it right.
    (The count-only call of ecb_csr_to_hapcsc_device reads nothing it could refuse; the filling call stands for the entry point.)"""
    import torch
    key = ENTRIES[entry][1][1]
    case = _case(entry, key)
    name, bad, code = case.bad
    slab, v = _place(case, "all4", extra=[(name + "~bad", bad, next(dt for n, _, dt in case.ins if n == name))])
    rc, _ = case.call(dict(v, **{name: v[name + "~bad"]}))
    torch.cuda.synchronize()
    assert rc == code, (rc, ecb.load().ecb_last_error(None))
    host = slab.host()
    for out, _, _ in case.outs:
        assert slab.untouched(out, host), out
    assert slab.check(host) == []
    _good_call(case, slab, v)


# ---- part 2: the entry points that take a handle ----------------------------------------------------------------------------------------
ALIGN_TEXT = b"device streams must be 16-byte aligned"
STREAMS = ("read_id", "locus", "hapflag")


def _i32(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("call", ["push_device", "push_device_tiled", "verify_device", "verify_device_tiled"])
def test_a_stream_off_16_bytes_is_refused_and_the_run_goes_on(call):
    """ecb.h asks for 16-byte alignment of the streams of ecb_push_device* and ecb_verify_device* and for nothing else.  Each pointer in
    turn at residue 4, then 8, then 12, the others on 16 bytes: ECB_ERR_ARG with the text that names the rule -- and, as for every bad
    argument, the run as it was: a first batch of whole reads pushed before, the second pushed after, finalize and export == the C oracle
    over both, the exactness pass counts 0.  (ecb_push_device on a handle with ECB_F_RANGES, so that ``pos`` is one of its pointers.)"""
    import torch
    t, T_, H_, exp = tps._short_stream()
    lib = ecb.load()
    n = len(t["read_id"])
    cut = int(np.searchsorted(t["read_id"], exp["n_reads"] // 2))
    ranges, tiled = call == "push_device", call.endswith("tiled")
    arr = {k: _i32(t[k]) for k in STREAMS}
    arr["pos"] = np.random.default_rng(3).integers(0, 1 << 30, size=n).astype(np.int32)
    names = STREAMS + (("pos",) if ranges else ())
    if tiled:
        tile = lambda a, z: ecb.tile_tuples(*[torch.from_numpy(arr[k][a:z]).cuda() for k in STREAMS]).cpu().numpy()   # noqa: E731
        parts = {"all": {"tiles": tile(0, n)}, "b1": {"tiles": tile(0, cut)}, "b2": {"tiles": tile(cut, n)}}
        names = ("tiles",)
    else:
        parts = {"all": {k: arr[k] for k in names}, "b1": {k: arr[k][:cut] for k in names}, "b2": {k: arr[k][cut:] for k in names}}
    slab = Slab("cuda", nbytes=1 << 22)
    v = {p: {k: slab.place("%s_%s" % (p, k), a, np.int32, 0, "in") for k, a in d.items()} for p, d in parts.items()}
    src = "all" if call.startswith("verify") else "b2"                   # (what the refused call is given)
    offs = {r: {k: slab.place("off%d_%s" % (r, k), parts[src][k], np.int32, r, "in") for k in names} for r in (4, 8, 12)}
    torch.cuda.synchronize()

    def push(b, p):
        if tiled:
            b.push_device_tiled(v[p]["tiles"], cut if p == "b1" else n - cut)
        else:
            b.push_device(*[v[p][k] for k in STREAMS], pos=v[p]["pos"] if ranges else None)

    with ecb.EcBuilder(T_, H_, track_ranges=ranges, **tps.SMALL) as b:
        push(b, "b1")
        before = b.counters()
        for r, k in ((r, k) for r in (4, 8, 12) for k in names):         # each pointer in turn, the others aligned
            p = {x: (offs[r] if x == k else v[src])[x] for x in names}
            assert p[k].data_ptr() % 16 == r and all(p[x].data_ptr() % 16 == 0 for x in names if x != k)
            bad, nl = C.c_uint64(77), C.c_uint64(77)
            if call == "push_device":
                rc = lib.ecb_push_device(b._h, _P(p["read_id"]), _P(p["locus"]), _P(p["hapflag"]), _P(p["pos"]), n - cut)
            elif call == "push_device_tiled":
                rc = lib.ecb_push_device_tiled(b._h, _P(p["tiles"]), n - cut)
            elif call == "verify_device":
                rc = lib.ecb_verify_device(b._h, _P(p["read_id"]), _P(p["locus"]), _P(p["hapflag"]), n, C.byref(bad), C.byref(nl))
            else:
                rc = lib.ecb_verify_device_tiled(b._h, _P(p["tiles"]), n, C.byref(bad), C.byref(nl))
            assert rc == ARG and ALIGN_TEXT in lib.ecb_last_error(b._h), (r, k, rc, lib.ecb_last_error(b._h))
            assert b.counters() == before, (r, k)
        push(b, "b2")
        s = b.finalize()
        _check(b.export(), s, exp)
        if tiled:
            assert b.verify_device_tiled(v["all"]["tiles"], n)[0] == 0
        else:
            assert b.verify_device(*[v["all"][k] for k in STREAMS])[0] == 0
    assert slab.check() == []


@pytest.mark.parametrize("tiled", [False, True], ids=["push_device", "push_device_tiled"])
def test_the_alignment_is_looked_at_before_the_open_read_of_a_host_push(tiled):
    """A host push leaves its last read open, and a device push is then out of order (ECB_ERR_STATE).  A device push whose stream is off
    16 bytes is a bad argument first: ECB_ERR_ARG and the text of the alignment rule at residues 8 and 12, ECB_ERR_STATE for the same
    call on aligned streams -- neither looks at a record, and the run goes on: the rest of the stream through the host push, finalize and
    export == the C oracle.  (Here a refusal that let 8 through would answer with the wrong code and still launch nothing.)"""
    import torch
    t, T_, H_, exp = tps._short_stream()
    lib = ecb.load()
    n = len(t["read_id"])
    cut = int(np.searchsorted(t["read_id"], exp["n_reads"] // 2))
    rest = {k: _i32(t[k][cut:]) for k in STREAMS}
    if tiled:
        rest = {"tiles": ecb.tile_tuples(*[torch.from_numpy(rest[k]).cuda() for k in STREAMS]).cpu().numpy()}
    slab = Slab("cuda", nbytes=1 << 21)
    v = {r: {k: slab.place("r%d_%s" % (r, k), a, np.int32, r, "in") for k, a in rest.items()} for r in (0, 8, 12)}

    def call(p):
        if tiled:
            return lib.ecb_push_device_tiled(b._h, _P(p["tiles"]), n - cut)
        return lib.ecb_push_device(b._h, _P(p["read_id"]), _P(p["locus"]), _P(p["hapflag"]), None, n - cut)
    with ecb.EcBuilder(T_, H_, **tps.SMALL) as b:
        b.push(*(t[k][:cut] for k in STREAMS))                           # (its last read stays open)
        for r in (8, 12):
            for k in rest:
                rc = call(dict(v[0], **{k: v[r][k]}))
                assert rc == ARG and ALIGN_TEXT in lib.ecb_last_error(b._h), (r, k, rc, lib.ecb_last_error(b._h))
        assert call(v[0]) == -6 and b"open read" in lib.ecb_last_error(b._h)
        b.push(*(t[k][cut:] for k in STREAMS))
        _check(b.export(), b.finalize(), exp)
    assert slab.check() == []


def _mk(T_, H_, **kw):
    return ecb.EcBuilder(T_, H_, ec_capacity=1 << 10, arena_capacity=1 << 24, **kw)


class _Placer(object):
    """Outputs placed in a slab as their sizes become known, 4-byte arrays at ``r4`` (4 or 12), 8-byte ones -- the 32-byte table entries
    and the 8-byte pairs, keys and hashes -- at 8; the slab checked after every call."""

    def __init__(self, r4, nbytes=1 << 24):
        self.slab, self.r4 = Slab("cuda", nbytes=nbytes), r4

    def out(self, name, n, dtype=np.int32):
        return self.slab.place(name, (max(int(n), 1),), dtype, 8 if np.dtype(dtype).itemsize == 8 else self.r4, "out")

    def inp(self, name, a, dtype=np.int32):
        return self.slab.place(name, a, dtype, 8 if np.dtype(dtype).itemsize == 8 else self.r4, "in")

    def clean(self, after):
        import torch
        torch.cuda.synchronize()
        assert self.slab.check() == [], after

    def read(self, t):
        return t.cpu().numpy()


def _export_device(pl, b, exp, tag):
    """ecb_export_device, all six arrays placed, == the C oracle."""
    s = b.sizes
    E, nnz = s["n_ecs"], s["nnz_a"]
    o = {"indptrA": pl.out(tag + "_ipa", E + 1), "indicesA": pl.out(tag + "_ixa", nnz), "dataA": pl.out(tag + "_daa", nnz),
         "indptrN": pl.out(tag + "_ipn", 2), "indicesN": pl.out(tag + "_ixn", E), "dataN": pl.out(tag + "_dan", E)}
    b._chk(b._lib.ecb_export_device(b._h, *[_P(o[k]) for k in ("indptrA", "indicesA", "dataA", "indptrN", "indicesN", "dataN")]))
    pl.clean("ecb_export_device " + tag)
    got = {k: pl.read(t) for k, t in o.items()}
    _check(dict(got, indicesA=got["indicesA"][:nnz], dataA=got["dataA"][:nnz]), s, exp)


@pytest.mark.parametrize("r4", [4, 12])
def test_tables_exported_merged_and_adopted_through_offset_views(r4):
    """Two shards of one stream: ecb_table_export_parts_device into placed entry and pair buffers (their room is ecb_table_sizes' upper
    bound: writing inside it is allowed, past it is not), ecb_table_merge_batch_device from slices of them (which it must not change),
    ecb_table_export_device of the merged ranges, ecb_table_adopt_batch_device, finalize, ecb_export_device == the C oracle (and so ==
    one handle over the whole stream)."""
    t, T_, H_, exp, R = tps._shard_stream()
    cut_reads, P = [0, R // 3, R], 2
    pl = _Placer(r4)
    pieces, counts, base = [], [], 0
    for k, b in enumerate(tps._shards(t, T_, H_, cut_reads)):
        ne, npairs, nreads = b.table_sizes()
        ent, prs = pl.out("ent%d" % k, ne * 4, np.int64), pl.out("prs%d" % k, npairs, np.int64)
        eo, po = b.table_export_parts_device(ent, prs, base, P)
        pl.clean("ecb_table_export_parts_device %d" % k)
        assert eo[-1] == ne and po[-1] <= npairs
        pl.slab.freeze("ent%d" % k); pl.slab.freeze("prs%d" % k)
        pieces.append((ent, prs, eo, po)); counts.append(b.counters()[:2]); base += nreads
        b.close()
    root, adopted = _mk(T_, H_), []
    for q in range(P):
        part = _mk(T_, H_)
        part.table_merge_batch_device([(ent[eo[q] * 4:eo[q + 1] * 4], eo[q + 1] - eo[q], prs[po[q]:po[q + 1]], po[q + 1] - po[q])
                                       for ent, prs, eo, po in pieces if eo[q + 1] > eo[q]])
        pl.clean("ecb_table_merge_batch_device %d" % q)
        pe_n, pp_n, _ = part.table_sizes()
        pe, pp = pl.out("pe%d" % q, pe_n * 4, np.int64), pl.out("pp%d" % q, pp_n, np.int64)
        part.table_export_device(pe, pp, 0)
        pl.clean("ecb_table_export_device %d" % q)
        pl.slab.freeze("pe%d" % q); pl.slab.freeze("pp%d" % q)
        adopted.append((pe, pe_n, pp, pp_n))
        part.close()
    root.table_adopt_batch_device(adopted)
    pl.clean("ecb_table_adopt_batch_device")
    root.add_counters(sum(c[0] for c in counts), sum(c[1] for c in counts), base)
    root.finalize()
    _export_device(pl, root, exp, "root")
    root.close()


@pytest.mark.parametrize("r4", [4, 12])
def test_ranges_rebased_finalized_and_assembled_through_offset_views(r4):
    """The other way round: entries exported from read 0 and moved on in place (ecb_table_rebase_device: the first reads change, nothing
    else does), every key range merged and finalized on a handle of its own, its piece written by ecb_export_device and
    ecb_export_firsts_device, the pieces put together by ecb_assemble_ranges_device (which must not change them), ecb_export_device
    == the C oracle."""
    t, T_, H_, exp, R = tps._shard_stream()
    cut_reads, P = [0, R // 3, R], 2
    pl = _Placer(r4)
    cuts, bases, base, totals = [], [], 0, [0, 0, 0]
    for k, b in enumerate(tps._shards(t, T_, H_, cut_reads)):
        ne, npairs, _ = b.table_sizes()
        ent, prs = pl.out("ent%d" % k, ne * 4, np.int64), pl.out("prs%d" % k, npairs, np.int64)
        eo, po = b.table_export_parts_device(ent, prs, 0, P)
        pl.clean("ecb_table_export_parts_device %d" % k)
        pl.slab.freeze("prs%d" % k)
        cuts.append((ent, prs, eo, po, pl.read(ent).reshape(-1, 4).copy())); bases.append(base)
        a, vv, nr = b.counters()
        totals = [totals[0] + a, totals[1] + vv, totals[2] + nr]
        base += nr
        b.close()
    ranges = []
    for q in range(P):
        part = _mk(T_, H_)
        tables = []
        for k, ((ent, prs, eo, po, was), rb) in enumerate(zip(cuts, bases)):
            if eo[q + 1] == eo[q]:
                continue
            sl = ent[eo[q] * 4:eo[q + 1] * 4]
            part.table_rebase_device(sl, eo[q + 1] - eo[q], rb)
            tables.append((sl, eo[q + 1] - eo[q], prs[po[q]:], po[q + 1] - po[q]))
        part.table_merge_batch_device(tables)
        pl.clean("ecb_table_rebase_device / ecb_table_merge_batch_device %d" % q)
        for k, ((ent, prs, eo, po, was), rb) in enumerate(zip(cuts, bases)):
            now = pl.read(ent).reshape(-1, 4)[eo[q]:eo[q + 1]]           # an entry: {u64 hash, u64 reserved, u32 count | u32 ~first << 32, u32 off | u32 n << 32}
            want = was[eo[q]:eo[q + 1]].copy()
            first = (~(want[:, 2] >> 32)) & 0xFFFFFFFF
            want[:, 2] = (want[:, 2] & 0xFFFFFFFF) | (((~(first + rb)) & 0xFFFFFFFF) << 32)
            assert np.array_equal(now.view(np.uint64), want.view(np.uint64)), (q, k)
        part.add_counters(*totals)
        s = part.finalize()
        E, nnz = s["n_ecs"], s["nnz_a"]
        ip, ix, da = pl.out("r%d_ip" % q, E + 1), pl.out("r%d_ix" % q, nnz), pl.out("r%d_da" % q, nnz)
        cn, fi = pl.out("r%d_cn" % q, E), pl.out("r%d_fi" % q, E)
        part.export_piece_device(ip, ix, da, cn, fi)
        pl.clean("ecb_export_device / ecb_export_firsts_device %d" % q)
        for nm in ("ip", "ix", "da", "cn", "fi"):
            pl.slab.freeze("r%d_%s" % (q, nm))
        ranges.append((ip, ix, da, cn, fi, E, nnz))
        part.close()
    root = _mk(T_, H_)
    root.assemble_ranges_device([p for p in ranges if p[5]], totals[2], totals[0], totals[1])
    pl.clean("ecb_assemble_ranges_device")
    _export_device(pl, root, exp, "root")
    root.close()


@pytest.mark.parametrize("r4", [4, 12])
def test_multisample_cells_keys_and_triples_through_offset_views(r4):
    """ecb_push_cells_device from a placed cell stream (one handle == the stream's own expectation), and the multi-GPU multisample
    protocol on placed buffers: ecb_export_ec_keys_device and ecb_export_device of the root, ecb_ms_local_triples_device of every shard
    (reads the keys and the CSR, writes key / count / first: room n_reads), ecb_ms_adopt_triples_device == the triples of one handle."""
    st, exp = tps._cached("ms_shards", lambda: (lambda s: (s, s.expected()))(tm._random_stream(np.random.default_rng(48), np.arange(300) * 5, 6000, 4, n_tpl=500)))
    tr, n_ecs = exp[0], exp[1]
    pl = _Placer(r4)
    # one handle, its cells from device memory
    meta = pl.inp("meta", _i32(st.meta))
    with ecb.EcBuilder(st.n_loci, tm.H, multisample=True, **tps.SMALL) as b:
        b.push(st.read_id, st.locus, st.hapflag)
        b.push_cells_device(meta, 0)
        tm._check_built(b, st, exp)
    pl.clean("ecb_push_cells_device")
    # shards: tables merged and adopted as everywhere else, then the triples through placed buffers
    cuts = [0, 2501, st.n_reads]
    shards, pieces, sizes, base = [], [], [], 0
    for k, (r0, r1) in enumerate(zip(cuts[:-1], cuts[1:])):
        b = ecb.EcBuilder(st.n_loci, tm.H, ec_capacity=1 << 12, multisample=True)
        b.push(*st.records(r0, r1))
        cells = pl.inp("cells%d" % k, _i32(st.meta[r0:r1]))
        b.push_cells_device(cells, 0)
        ne, npairs, nreads = b.table_sizes()
        ent, prs = pl.out("ent%d" % k, ne * 4, np.int64), pl.out("prs%d" % k, npairs, np.int64)
        eo, po = b.table_export_parts_device(ent, prs, base, 1)
        pl.clean("ecb_table_export_parts_device %d" % k)
        pieces.append((ent, eo[1], prs, po[1])); sizes.append((nreads,) + b.counters()[:2]); shards.append((b, base))
        base += nreads
    part = ecb.EcBuilder(st.n_loci, tm.H, ec_capacity=1 << 12)
    part.table_merge_batch_device(pieces)
    pe_n, pp_n, _ = part.table_sizes()
    pe, pp = pl.out("pe", pe_n * 4, np.int64), pl.out("pp", pp_n, np.int64)
    part.table_export_device(pe, pp, 0)
    part.close()
    root = ecb.EcBuilder(st.n_loci, tm.H, ec_capacity=1 << 12, multisample=True)
    root.table_adopt_batch_device([(pe, pe_n, pp, pp_n)])
    root.add_counters(sum(s[1] for s in sizes), sum(s[2] for s in sizes), base)
    s = root.finalize()
    E, nnz = s["n_ecs"], s["nnz_a"]
    keys, ip, ix, da = pl.out("keys", E, np.int64), pl.out("ip", E + 1), pl.out("ix", nnz), pl.out("da", nnz)
    root.export_ec_keys_device(keys)
    root.export_device(ip, ix, da)
    pl.clean("ecb_export_ec_keys_device / ecb_export_device")
    for nm in ("keys", "ip", "ix", "da"):
        pl.slab.freeze(nm)
    tables = []
    for k, (b, b0) in enumerate(shards):
        nreads = b.table_sizes()[2]
        key, cnt, first = pl.out("key%d" % k, nreads, np.int64), pl.out("cnt%d" % k, nreads), pl.out("first%d" % k, nreads)
        n = b.ms_local_triples_device(keys, ip, ix, da, E, b0, key, cnt, first)
        pl.clean("ecb_ms_local_triples_device %d" % k)
        assert 0 < n <= nreads
        for nm in ("key", "cnt", "first"):
            pl.slab.freeze("%s%d" % (nm, k))
        tables.append((key, cnt, first, n))
    root.ms_adopt_triples_device(tables)
    pl.clean("ecb_ms_adopt_triples_device")
    try:
        got = root.export_pairs()
        for k in ("ec", "cell", "file", "count", "first"):
            assert np.array_equal(got[k], tr[k]), k
        a = root.export()
        for k, e in zip(("indptrA", "indicesA", "dataA"), exp[2]):
            assert np.array_equal(a[k], e), k
    finally:
        root.close()
        for b, _ in shards:
            b.close()
