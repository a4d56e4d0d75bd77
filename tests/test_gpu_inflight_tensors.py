"""Every tensor path of the Python layer on caller memory WHEN a caller calls (``tests/inflight.py``; where it sits:
``test_gpu_caller_views*.py``): inputs that a kernel queued on torch's current stream has not written yet, outputs whose fill is still
queued, a current stream that is not the default one, and memory that torch reuses the moment the call returns.

include/ecb.h wants finished inputs and works on streams of its own.  Those order themselves behind torch's default stream (the legacy
null stream) and behind no other, so the Python layer waits for a current stream that is not the default one: ``_Torch.ready()`` for
the one-call wrappers, ``EcBuilder._device_call`` for the handle ("Streams").

One case = one entry point in one mode:

* ``off``: nothing in flight -- the case itself.
* ``default-late``: the producer (a delay, then the real content over a decoy) is queued on the default stream, in flight on the line
  before the call.
* ``default-converted-i64 / -strided / -cpu``: the same, with the inputs handed over as the wrapper must convert them, so that the
  binding's own ``.to().contiguous()`` is the producer that is queued behind the delay.  (``-cpu``: the second array is a CPU tensor;
  torch's copy of it waits for the stream it is queued on, so this mode holds the wrapper to the result and to ``reuse_after`` only.)
* ``side-late``, ``side-converted-*``: the same inside ``with torch.cuda.stream(torch.cuda.Stream())``.

The handle's ``*_device`` methods take pointers as they are and convert nothing: they run ``off``, ``default-late`` and ``side-late``.
An *output* of theirs is late too: its fill (0x5C over 0xA5) is queued behind the delay, as a caller's ``zeros()`` would be.

After every call: it returned; the result bit for bit against the checker the entry point's own GPU test uses (the ecquant family:
bit for bit against the same call on finished tensors, which the existing tests hold to their reference), and against that finished
call for every entry; ``reuse_after``'s clones equal it too; the decoy's own answer differs from the real one on the CPU checker.
A layer that ignores the ordering computes the decoy's answer, a valid one, and the comparison fails: nothing here may fault."""
import copy
import time

import numpy as np
import pytest

from alntools_amd import ecb, ecb_boot, ecb_bus, ecb_bus_correct, ecb_components, ecb_strata, ecb_umi

import boot_checker as bc
import bundle_checker as bchk
import bus_checker as busc
import bus_correct_checker as cc
import cell_model_checker as cmchk
import cell_quant_checker as cq
import components_checker
import counts_checker
import ec_merge_checker as chk
import gt_checker
import inflight as fl
import post_checker as pchk
import quant_checker as qchk
import quant_model_checker as mchk
import salmon_checker as schk
import select_checker
import strata_checker as sk
import umi_checker as uc
from inflight import Input

pytestmark = pytest.mark.gpu

ITERS = 3                        # every iterative entry: a few steps, tol 0, so that no call takes longer than the rest
SEED, B0, B = 9, 2, 3
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _cv():
    import test_gpu_caller_views as cv
    return cv


class Entry(object):
    """``inputs``: [Input]; ``outs``: [(name, shape, numpy dtype)] the caller allocates; ``prepare()`` -> state, before anything is in
    flight (a handle with its host pushes done); ``call(v, state)`` -> what the call returned, made while the producer is in flight;
    ``finish(out, state)`` -> the result, after ``reuse_after``; ``want(arrays)`` -> the checker's result for those input arrays, a list
    that ``exact`` entries equal bit for bit from its first element on (the others: the checker only says that the decoy's answer differs)."""

    def __init__(self, inputs, call, want, exact=True, outs=(), prepare=None, finish=None, env=None):
        self.inputs, self.call, self.want, self.exact, self.outs = inputs, call, want, exact, list(outs)
        self.prepare, self.finish, self.env, self.plain = prepare or (lambda: None), finish or (lambda out, state: out), env, finish is None


def _i32(xs):
    return [np.ascontiguousarray(x, dtype=np.int32) for x in xs]


# ---- the matrices of test_gpu_caller_views.py and their decoys ---------------------------------------------------------------------------
def _matrix(zeros=1):
    cv = _cv()
    return cv._matrix(1, zeros), cv.T, cv.H, cv.S


def _decoys(m, H, seed, zeros):
    """Other valid masks and other valid counts for the non-zeros of A and N (``zeros``: some of them 0, at other places than m's)."""
    rng = np.random.default_rng(seed)
    da = rng.integers(1, 1 << H, size=len(m.dataA), dtype=np.int64)
    dn = rng.integers(1, 40, size=len(m.dataN), dtype=np.int64)
    if zeros:
        da[rng.random(len(da)) < 0.05] = 0
        dn[rng.random(len(dn)) < 0.03] = 0
    return da.astype(np.int32), dn.astype(np.int32)


def _six(m, da=None, dn=None):
    """The six arrays as inputs: the arrays that index keep their content, the masks and the counts have a decoy where one is given."""
    return [Input("ip", m.indptrA, wide=True), Input("ix", m.indicesA, wide=True), Input("da", m.dataA, da, wide=True),
            Input("pn", m.indptrN, wide=True), Input("xn", m.indicesN, wide=True), Input("dn", m.dataN, dn, wide=True)]


def _mats(a, T, H):
    return (a["ip"], a["ix"], a["da"], T, H, a["pn"], a["xn"], a["dn"])


def _with(m, a, pre=""):
    """``m`` with the masks and counts of the arrays ``a``."""
    m2 = copy.copy(m)
    m2.dataA, m2.dataN = np.asarray(a[pre + "da"], dtype=m.dataA.dtype), np.asarray(a[pre + "dn"], dtype=m.dataN.dtype)
    return m2


def _tables(T, H, seed):
    rng = np.random.default_rng(seed)
    theta = [rng.random((H, T)) * 10 + 0.01 for _ in range(2)]
    scale = [1.0 / rng.integers(1, 3000, size=(H, T)) for _ in range(2)]
    return theta, scale


def _gene(T, n_genes=97):
    return (np.arange(T) * 7 % n_genes).astype(np.int32), n_genes


def _rot(mask, H):
    """Every mask rotated by one haplotype: another valid mask with as many set bits."""
    mask = np.asarray(mask, dtype=np.int64)
    return (((mask << 1) | (mask >> (H - 1))) & ((1 << H) - 1)).astype(np.int32)


def _info(i):
    return [i[k] for k in sorted(i)]


# ---- the conversions --------------------------------------------------------------------------------------------------------------------
def entry_csr_to_hapcsc():
    m, T, H, _ = _matrix(0)
    da, _ = _decoys(m, H, 1, 0)
    ins = _six(m, da)[:3]

    def want(a):
        lay = pchk.Layout(a["ip"], a["ix"], a["da"], T, H)
        return [lay.csc_indptr, lay.csc_indices]
    return Entry(ins, lambda v, _: ecb.csr_to_hapcsc(v["ip"], v["ix"], v["da"], T, H), want)


def entry_csr_to_hapcsc_values():
    """(the values are one per set bit: the decoy masks have as many as the real ones, whichever of the two a non-zero holds)"""
    m, T, H, _ = _matrix(0)
    n_bits = int(np.unpackbits(m.dataA.view(np.uint8)).sum())
    rng = np.random.default_rng(2)
    ins = _six(m, _rot(m.dataA, H))[:3] + [Input("va", rng.random(n_bits), rng.random(n_bits) + 2)]

    def want(a):
        lay = pchk.Layout(a["ip"], a["ix"], a["da"], T, H)
        return [lay.csc_indptr, lay.csc_indices, lay.to_csc(a["va"])]
    return Entry(ins, lambda v, _: ecb.csr_to_hapcsc_values(v["ip"], v["ix"], v["da"], v["va"], T, H), want)


def _csr_of_hapcsc(cp, ci, E, T, H):
    """A = the sum over h of 2^h M_h as CSR, columns ascending (``bin_utils.emase2ec``)."""
    keys, bits, at = [], [], 0
    for h in range(H):
        n = int(cp[h, -1])
        col = np.repeat(np.arange(T, dtype=np.int64), np.diff(cp[h].astype(np.int64)))
        keys.append(ci[at:at + n].astype(np.int64) * T + col)
        bits.append(np.full(n, 1 << h, dtype=np.int64))
        at += n
    key, inv = np.unique(np.concatenate(keys), return_inverse=True)
    mask = np.zeros(len(key), dtype=np.int64)
    np.bitwise_or.at(mask, inv, np.concatenate(bits))
    return _i32([np.concatenate([[0], np.cumsum(np.bincount(key // T, minlength=E))]), key % T, mask])


def entry_hapcsc_to_csr():
    """This entry point has no value array: its arrays are structure.  The decoy is the per-haplotype CSC of the same matrix with every
    mask rotated by one haplotype -- a valid input of the same sizes, the planes permuted."""
    m, T, H, _ = _matrix(0)
    lay, rot = pchk.Layout(m.indptrA, m.indicesA, m.dataA, T, H), pchk.Layout(m.indptrA, m.indicesA, _rot(m.dataA, H), T, H)
    E = m.num_reads
    ins = [Input("cp", lay.csc_indptr, rot.csc_indptr, wide=True), Input("ci", lay.csc_indices, rot.csc_indices, wide=True)]
    assert _csr_of_hapcsc(lay.csc_indptr, lay.csc_indices, E, T, H)[2].tobytes() == m.dataA.astype(np.int32).tobytes()
    return Entry(ins, lambda v, _: ecb.hapcsc_to_csr(v["cp"], v["ci"], E), lambda a: _csr_of_hapcsc(a["cp"], a["ci"], E, T, H))


def entry_apply_mask():
    m, T, H, _ = _matrix(1)
    da, _ = _decoys(m, H, 3, 1)
    rng = np.random.default_rng(4)
    mask = [rng.integers(0, 1 << H, size=T, dtype=np.int64).astype(np.int32) for _ in range(2)]
    ins = _six(m, da)[:3] + [Input("mask", mask[0], mask[1], wide=True)]
    return Entry(ins, lambda v, _: ecb.apply_mask(v["ip"], v["ix"], v["da"], v["mask"], H),
                 lambda a: _i32(gt_checker.mask_csr(a["ip"], a["ix"], a["da"], a["mask"].view(np.uint32))))


def entry_count_alignments():
    m, T, H, _ = _matrix(1)
    ins = _six(m, *_decoys(m, H, 5, 1))
    return Entry(ins, lambda v, _: ecb.count_alignments(*_mats(v, T, H), sample=2),
                 lambda a: [np.asarray(x, dtype=np.int64) for x in counts_checker.count(*_mats(a, T, H), sample=2)])


# ---- ecquant ----------------------------------------------------------------------------------------------------------------------------
def _quant_inputs(seed, theta_name="th"):
    m, T, H, S = _matrix(1)
    _, dn = _decoys(m, H, seed, 1)
    theta, scale = _tables(T, H, seed)
    return m, T, H, S, _six(m, None, dn) + [Input("sc", scale[0], scale[1]), Input(theta_name, theta[0], theta[1])]


def entry_quantify():
    m, T, H, S, ins = _quant_inputs(6)

    def want(a):
        theta, info = qchk.run(qchk.Problem(*_mats(a, T, H)), a["sc"], a["th"], ITERS, 0.0)
        return [theta] + _info(info)
    return Entry(ins, lambda v, _: ecb.quantify(*_mats(v, T, H), scale=v["sc"], theta_in=v["th"], max_iters=ITERS, tol=0.0), want, exact=False)


def entry_quantify_model():
    m, T, H, S, ins = _quant_inputs(7)
    gene, G = _gene(T)
    ins.append(Input("gene", gene, wide=True))

    def want(a):
        theta, info = mchk.run(mchk.Grouping(qchk.Problem(*_mats(a, T, H)), a["gene"], G), 1, a["sc"], a["th"], ITERS, 0.0)
        return [theta] + _info(info)
    return Entry(ins, lambda v, _: ecb.quantify_model(*_mats(v, T, H), v["gene"], G, 1, scale=v["sc"], theta_in=v["th"], max_iters=ITERS, tol=0.0),
                 want, exact=False)


def entry_posterior():
    m, T, H, S = _matrix(0)
    theta, scale = _tables(T, H, 8)
    ins = _six(m)[:3] + [Input("th", theta[0], theta[1]), Input("sc", scale[0], scale[1])]
    p, lay = qchk.Problem.of(m), pchk.Layout.of(m)

    def want(a):
        post, mass = pchk.posterior(p, lay, 4, a["th"], a["sc"])
        return [post, lay.bit_ptr, mass]
    return Entry(ins, lambda v, _: ecb.posterior(v["ip"], v["ix"], v["da"], T, H, v["th"], scale=v["sc"]), want, exact=False)


def _keep(S):
    keep = np.ones(S, dtype=bool)
    keep[[1, 8]] = False
    return keep


def entry_cell_support():
    m, T, H, S = _matrix(1)
    ins = _six(m, *_decoys(m, H, 9, 1))
    keep = _keep(S)

    def want(a):
        ptr, loc = cq.expected_support(cq.cells(_with(m, a), keep))
        return [np.asarray(ptr, dtype=np.int64), np.asarray(loc, dtype=np.int32)]
    return Entry(ins, lambda v, _: ecb.cell_support(*_mats(v, T, H), cell_keep=keep), want)


def entry_quantify_cells():
    m, T, H, S, ins = _quant_inputs(10)
    keep = _keep(S)

    def want(a):
        ptr, loc, theta, info = cq.quantify_cells(*_mats(a, T, H), cell_keep=keep, scale=a["sc"], theta_in=a["th"], max_iters=ITERS, tol=0.0)
        return [ptr, loc, theta] + _info(info)
    return Entry(ins, lambda v, _: ecb.quantify_cells(*_mats(v, T, H), cell_keep=keep, scale=v["sc"], theta_in=v["th"], max_iters=ITERS, tol=0.0),
                 want, exact=False)


def entry_quantify_cells_model():
    m, T, H, S, ins = _quant_inputs(11)
    gene, G = _gene(T)
    ins.append(Input("gene", gene, wide=True))

    def want(a):
        ptr, loc, theta, info = cmchk.quantify_cells_model(*_mats(a, T, H), a["gene"], G, 3, scale=a["sc"], theta_in=a["th"], max_iters=ITERS, tol=0.0)
        return [ptr, loc, theta] + _info(info)
    return Entry(ins, lambda v, _: ecb.quantify_cells_model(*_mats(v, T, H), v["gene"], G, 3, scale=v["sc"], theta_in=v["th"], max_iters=ITERS,
                                                            tol=0.0), want, exact=False)


def entry_resample():
    m, T, H, S = _matrix(1)
    _, dn = _decoys(m, H, 12, 1)
    ins = _six(m, None, dn)[3:]
    E = m.num_reads
    return Entry(ins, lambda v, _: ecb_boot.resample(E, v["pn"], v["xn"], v["dn"], sample=4, seed=SEED, b0=B0, n_reps=B),
                 lambda a: list(bc.resample(bc.weights(E, a["pn"], a["xn"], a["dn"], 4), SEED, B0, B)[:3]))


def entry_quantify_bootstrap():
    """(the checker's part here: the replicates the EMs run on differ between the real counts and the decoy's, and so does the scale)"""
    m, T, H, S = _matrix(1)
    _, dn = _decoys(m, H, 13, 1)
    _, scale = _tables(T, H, 13)
    ins = _six(m, None, dn) + [Input("sc", scale[0], scale[1])]
    E = m.num_reads

    def call(v, _):
        return ecb_boot.quantify_bootstrap(*_mats(v, T, H), B, seed=SEED, scale=v["sc"], max_iters=ITERS, tol=0.0, return_reps=True)
    return Entry(ins, call, lambda a: list(bc.resample(bc.weights(E, a["pn"], a["xn"], a["dn"]), SEED, 0, B)[:3]) + [a["sc"]], exact=False)


# ---- the .bin to .bin entry points ------------------------------------------------------------------------------------------------------
def _bin_of(exp):
    return _i32([exp.indptrA, exp.indicesA, exp.dataA, exp.indptrN, exp.indicesN, exp.dataN])


def entry_combine():
    cv = _cv()
    m0, T, H, S = _matrix(0)
    cv.case_combine(1)                                                        # (makes and caches the second part and the plan)
    m1, plan, _ = cv._CACHE[("combine", 1)]
    ins = []
    for k, (m, tmap, smap, seed) in enumerate(zip((m0, m1), (None, plan.target_maps[1]), plan.sample_maps, (14, 15))):
        da, dn = _decoys(m, H, seed, 0)
        ins += [Input("p%d_%s" % (k, i.name), i.real, None if i.decoy is i.real else i.decoy, wide=True) for i in _six(m, da if k else None, dn)]
        ins += [Input("p%d_tm" % k, np.asarray(tmap, dtype=np.int32), wide=True)] if tmap is not None else []
        ins += [Input("p%d_sm" % k, np.asarray(smap, dtype=np.int32), wide=True)]
    n_samples = len(plan.sname)

    def call(v, _):
        parts = [dict(indptrA=v[p + "ip"], indicesA=v[p + "ix"], dataA=v[p + "da"], indptrN=v[p + "pn"], indicesN=v[p + "xn"], dataN=v[p + "dn"],
                      n_loci=T, target_map=v.get(p + "tm"), sample_map=v[p + "sm"]) for p in ("p0_", "p1_")]
        return ecb.combine(parts, T, H, n_samples)
    return Entry(ins, call, lambda a: _bin_of(chk.merge([_with(m0, a, "p0_"), _with(m1, a, "p1_")])))


def entry_bundle():
    import test_gpu_ecbundle as tb
    m, T, H, S = _matrix(0)
    groups = tb._grouping("mixed", np.random.default_rng(1), T)
    mp, mi = bchk.group_csr(T, groups)
    ins = _six(m, *_decoys(m, H, 16, 0)) + [Input("mp", mp.astype(np.int32), wide=True), Input("mi", mi.astype(np.int32), wide=True)]
    return Entry(ins, lambda v, _: ecb.bundle(v["ip"], v["ix"], v["da"], v["pn"], v["xn"], v["dn"], T, H, len(groups), v["mp"], v["mi"]),
                 lambda a: _bin_of(bchk.bundle(_with(m, a), tb._names(len(groups)), groups)))


def entry_select():
    m, T, H, S = _matrix(1)
    ins = _six(m, *_decoys(m, H, 17, 1))
    keep = _keep(S)

    def want(a):
        exp, stay, _ = select_checker.select_flags(_with(m, a), "unique", keep, 3)
        return _bin_of(exp) + [np.asarray(stay, dtype=bool)]
    return Entry(ins, lambda v, _: ecb.select(v["ip"], v["ix"], v["da"], v["pn"], v["xn"], v["dn"], T, H, row_class="unique", sample_keep=keep,
                                              min_count=3), want)


def entry_salmon_ecs():
    """(payload bytes of equal layout: the same lines with the last digit of every count another digit)"""
    rng = np.random.default_rng(52)
    names = schk.target_names(150, ["h%d" % h for h in range(4)], rng)
    n_ecs = 3000
    ptr, tid, counts = schk.random_ecs(rng, len(names), n_ecs, mean_k=6.0, long_every=50, long_k=(50, 400))
    counts = np.asarray(counts, dtype=np.int64)
    other = counts - counts % 10 + (counts % 10 + 1 + rng.integers(0, 8, size=len(counts))) % 10
    lname, hname, col, hap = schk.number_names(names)
    eff = rng.uniform(0, 5000, size=len(names))
    text, decoy = (np.frombuffer(schk.ec_section(ptr, tid, c), dtype=np.uint8) for c in (counts, other))
    assert len(text) == len(decoy) and np.array_equal(text == 9, decoy == 9) and np.array_equal(text == 10, decoy == 10)
    of = {text.tobytes(): counts, decoy.tobytes(): other}

    def want(a):
        exp = schk.expected(names, eff, ptr, tid, of[a["text"].tobytes()])
        return _i32([exp[3], exp[4], exp[5], exp[7], exp[8]])
    return Entry([Input("text", text, decoy)], lambda v, _: ecb.salmon_ecs(v["text"], n_ecs, col, hap, len(lname), len(hname)), want)


def entry_components():
    m, T, H, S = _matrix(1)
    ins = _six(m, *_decoys(m, H, 18, 1))
    return Entry(ins, lambda v, _: ecb_components.components(*_mats(v, T, H), min_count=25),
                 lambda a: (lambda r: list(r[:5]) + list(r[5]))(components_checker.components(*_mats(a, T, H), min_count=25)))


# ---- BUS --------------------------------------------------------------------------------------------------------------------------------
def entry_bus_molecules():
    """(payload bytes of equal layout: the same barcodes, other UMIs, ECs, counts and flags; the capacities are the header's bounds for
    any mixture of the two, handed over so that the wrapper has no reason to read a tensor back)"""
    import test_gpu_caller_views_bus as tvb
    rec, lines, cells = tvb._input()
    n = tvb.N_REC
    rng = np.random.default_rng(19)
    barcodes = rec.reshape(-1, 32)[:, :8].copy().view("<u8").reshape(-1)
    decoy = busc.records(barcodes, rng.integers(0, 150, size=n).astype(np.uint64), rng.integers(0, 50, size=n), rng.integers(0, 4, size=n))
    keep = cells[[0, 2, 3, 5, 8]]
    ptr, ids = busc.csr_lines(lines)
    caps = (len(keep), n, n * max(len(x) for x in lines), n)
    T, H, tcol, thap = tvb.T, tvb.H, tvb.TCOL, tvb.THAP
    ins = [Input("rec", rec.reshape(-1), decoy.reshape(-1)), Input("ptr", ptr.astype(np.int32), wide=True), Input("ids", ids.astype(np.int32), wide=True),
           Input("tcol", tcol.astype(np.int32), wide=True), Input("thap", thap.astype(np.int32), wide=True), Input("keep", keep)]

    def want(a):
        w = busc.molecules(a["rec"].reshape(-1, 32), lines, tcol, thap, keep=keep)
        return ([np.array(w.barcodes, dtype=np.uint64)] + _i32(busc.csr(w.rows)) + _i32(busc.csc(w.N, w.sizes[0])) + [np.array(w.row_line, dtype=np.int32)]
                + list(w.sizes))
    return Entry(ins, lambda v, _: ecb_bus.molecules(v["rec"], 12, 8, v["ptr"], v["ids"], v["tcol"], v["thap"], T // H, H, keep=v["keep"], capacities=caps),
                 want)


def entry_bus_correct():
    """(payload bytes of equal layout: the same records with the barcodes drawn again)"""
    import test_gpu_caller_views_bus_correct as tvc
    rec, white, _, _ = tvc._input()
    rng = np.random.default_rng(20)
    decoy = rec.reshape(-1, 32).copy()
    decoy[:, :8] = decoy[rng.permutation(len(decoy)), :8]

    def want(a):
        status, kept, sizes = cc.correct(a["rec"].reshape(-1, 32), tvc.BCLEN, white)
        return [kept, status] + list(sizes)
    return Entry([Input("rec", rec.reshape(-1), decoy.reshape(-1)), Input("white", white)],
                 lambda v, _: ecb_bus_correct.correct(v["rec"], tvc.BCLEN, v["white"], want_status=True), want)


# ---- the tuple streams -------------------------------------------------------------------------------------------------------------------
def _strata(inplace):
    """(``read_id`` and ``hapflag`` say where reads begin and which records pass: they index, and keep their content; the scores differ)"""
    import test_gpu_caller_views_strata as tvs
    rid, hf, sc, _, _ = tvs._input()
    other = np.random.default_rng(21).permutation(sc)
    ins = [Input("rid", rid, fixed=inplace, wide=True), Input("hf", hf, fixed=inplace, wide=True), Input("sc", sc, other, wide=True)]

    def want(a):
        out_rid, out_hf, counts = sk.best_strata(a["rid"], a["hf"], a["sc"])
        return [out_rid, out_hf] + list(counts)
    return Entry(ins, lambda v, _: ecb_strata.best_strata(v["rid"], v["hf"], v["sc"], inplace=inplace), want)


def entry_best_strata():
    return _strata(False)


def entry_best_strata_inplace():
    return _strata(True)


def entry_collapse_umis():
    """(the three streams index; the keys say which reads are one molecule: the decoy deals the same keys out to other reads)"""
    import test_gpu_caller_views_umi as tvu
    rid, loc, hf, keys, _, _ = tvu._input()
    other = np.random.default_rng(22).permutation(keys)
    ins = [Input("rid", rid, wide=True), Input("loc", loc, wide=True), Input("hf", hf, wide=True), Input("key", keys, other)]

    def want(a):
        r = uc.collapse(a["rid"], a["loc"], a["hf"], a["key"])
        return list(r[:4]) + list(r[4])
    return Entry(ins, lambda v, _: ecb_umi.collapse_umis(v["rid"], v["loc"], v["hf"], v["key"], tvu.N_LOCI, tvu.N_HAPS), want)


# ---- the handle -------------------------------------------------------------------------------------------------------------------------
SMALL = dict(ec_capacity=1 << 12, arena_capacity=1 << 24)
STREAMS = ("read_id", "locus", "hapflag")


def _short():
    import test_gpu_poisoned_scratch as tps
    return tps._short_stream()


def _stream_inputs():
    """3 000 reads of up to 12 records: the read ids index; the loci move on by one target and the haplotypes by one (other valid ones)."""
    t, T, H, exp = _short()
    hap, flg = t["hapflag"] >> 16, t["hapflag"] & 0xFFFF
    return t, T, H, exp, [Input("read_id", t["read_id"]), Input("locus", t["locus"], (t["locus"] + 1) % T),
                          Input("hapflag", t["hapflag"], (((hap + 1) % H) << 16 | flg).astype(np.uint32))]


def _oracle(a, H):
    import test_gpu_thresholds as th
    exp = th._oracle({k: np.ascontiguousarray(a[k]).view(np.uint32) for k in STREAMS}, H)
    n = len(exp["count"])
    return _i32([exp["indptr"], exp["indices"], exp["data"], [0, n], np.arange(n), exp["count"]]) + [n, exp["n_all"], exp["n_valid"], exp["n_reads"]]


def _exported(b):
    s = b.finalize()
    out = b.export()
    return [out[k] for k in ("indptrA", "indicesA", "dataA", "indptrN", "indicesN", "dataN")] + [s[k] for k in ("n_ecs", "all_alignments", "valid_alignments",
                                                                                                                 "n_reads")]


def _closing(fn):
    """``fn`` as an entry's ``finish`` whose state is its handle: closed afterwards."""
    def finish(out, b):
        try:
            return fn(out, b)
        finally:
            b.close()
    return finish


def _push(how, compilation="std"):
    import test_gpu_thresholds as th
    t, T, H, exp, ins = _stream_inputs()
    env, hinted, kernel = th.COMPILATIONS[compilation]
    n = len(t["read_id"])

    def prepare():
        b = ecb.EcBuilder(T, H, **SMALL)
        if hinted:
            b.hint_reads(exp["n_reads"])
        return b

    def call(v, b):
        if how == "tiled":                                                  # (tile_tuples' own copies are queued behind the producer too)
            b.push_device_tiled(ecb.tile_tuples(*[v[k] for k in STREAMS]), n)
        else:
            b.push_device(*[v[k] for k in STREAMS])
        return b

    def finish(b, state):
        assert b.profile_kernel().startswith(kernel), b.profile_kernel()
        return _exported(b)
    return Entry(ins, call, lambda a: _oracle(a, H), prepare=prepare, finish=_closing(finish), env=env)


def entry_verify_device():
    """(the handle holds the real stream; the pass over the decoy's loci and haplotypes finds its reads in wrong ECs)"""
    import verify_checker
    t, T, H, exp, ins = _stream_inputs()

    def prepare():
        b = ecb.EcBuilder(T, H, **SMALL)
        b.push(*(t[k] for k in STREAMS))
        b.finalize()
        return b

    def want(a):
        return [int(verify_checker.misplaced(t, {k: np.ascontiguousarray(a[k]).view(np.uint32) for k in STREAMS}, H).sum())]
    return Entry(ins, lambda v, b: (b, b.verify_device(*[v[k] for k in STREAMS])), want, prepare=prepare, finish=_closing(lambda out, b: out[1]))


def entry_push_cells_device():
    """ecb.h: ``d_meta`` stays alive and unchanged until the next call that waits for the handle -- ``call`` makes that call
    (``finalize``) before it returns, and ``reuse_after`` comes behind it.  The decoy: the same reads in other cells and files."""
    import test_gpu_multisample as tm
    st = _cached("ms_stream", lambda: tm._random_stream(np.random.default_rng(48), np.arange(300) * 5, 6000, 4, n_tpl=500))
    other = (np.random.default_rng(23).permutation(st.cell) | (st.file << 22)).astype(np.uint32)       # (every read stays in its file)
    n_cells = 1500

    def prepare():
        b = ecb.EcBuilder(st.n_loci, tm.H, multisample=True, **SMALL)
        b.push(st.read_id, st.locus, st.hapflag)
        b.counters()
        return b

    def call(v, b):
        b.push_cells_device(v["meta"], 0)
        b.finalize()
        return b

    def finish(b, state):
        pairs, f = b.export_pairs(), b.ms_filter(n_cells, 3)
        return [pairs[k] for k in ("ec", "cell", "file", "count", "first")] + [f[k] for k in ("kept_cells", "indptrA", "indicesA", "dataA", "indptrN", "indicesN",
                                                                                              "dataN", "n_cells_seen")]

    def want(a):
        from ms_checker import reduce_triples, select_rows
        meta = np.ascontiguousarray(a["meta"]).view(np.uint32).astype(np.int64)
        tr, n_ecs, (ip, ix, da) = tm.Stream(st.tpl, meta & ((1 << 22) - 1), meta >> 22).expected()
        kept, ec_keep, (n_ptr, n_idx, n_dat) = reduce_triples(tr, n_ecs, n_cells, 3)
        return [tr[k] for k in ("ec", "cell", "file", "count", "first")] + [np.asarray(kept, dtype=np.uint32)] + _i32(
            list(select_rows(ip, ix, da, ec_keep)) + [n_ptr, n_idx, n_dat]) + [len(np.unique(tr["cell"]))]
    return Entry([Input("meta", st.meta, other)], call, want, prepare=prepare, finish=_closing(finish))


def _export(which):
    """A finalized handle's results into caller tensors.  ``csr`` (``export_device``), ``keys`` (``export_ec_keys_device``) and ``piece``
    (``export_piece_device``): the outputs' fill is still queued when the call is made; == the C oracle, the keys == the numpy set hash.
    ``assemble``: that piece through ``assemble_ranges_device`` with counts that are late (the decoy: every count one more), finalize
    and export == the C oracle."""
    import set_hash
    t, T, H, exp = _short()
    E, nnz = len(exp["count"]), len(exp["indices"])
    count = exp["count"].astype(np.int32)
    a_csr = _i32([exp["indptr"], exp["indices"], exp["data"]])
    csr_outs = [("ip", (E + 1,), np.int32), ("ix", (nnz,), np.int32), ("da", (nnz,), np.int32)]
    outs = {"csr": csr_outs, "keys": [("keys", (E,), np.int64)], "piece": csr_outs + [("cn", (E,), np.int32), ("fi", (E,), np.int32)], "assemble": []}[which]

    def prepare():
        import torch
        b = ecb.EcBuilder(T, H, **SMALL)
        b.push(*(t[k] for k in STREAMS))
        b.finalize()
        if which != "assemble":
            return b
        piece = [torch.zeros(n, dtype=torch.int32, device="cuda") for n in (E + 1, nnz, nnz, E, E)]
        torch.cuda.synchronize()
        b.export_piece_device(*piece)
        torch.cuda.synchronize()
        return {"b": b, "piece": piece, "root": ecb.EcBuilder(T, H, **SMALL)}

    def call(v, state):
        if which == "csr":
            state.export_device(v["ip"], v["ix"], v["da"])
        elif which == "keys":
            state.export_ec_keys_device(v["keys"])
        elif which == "piece":
            state.export_piece_device(v["ip"], v["ix"], v["da"], v["cn"], v["fi"])
        else:
            ip, ix, da, _, fi = state["piece"]
            state["root"].assemble_ranges_device([(ip, ix, da, v["cn"], fi, E, nnz)], exp["n_reads"], exp["n_all"], exp["n_valid"])
            return []
        return [v[n] for n, _, _ in outs]

    def finish(out, state):
        if which != "assemble":
            state.close()
            return out
        try:
            return _exported(state["root"])
        finally:
            state["root"].close()
            state["b"].close()

    def want(a):
        if which == "assemble":
            return a_csr + _i32([[0, E], np.arange(E), a["cn"]]) + [E, exp["n_all"], exp["n_valid"], exp["n_reads"]]
        return {"csr": a_csr, "keys": [set_hash.row_hashes(exp["indptr"], exp["indices"], exp["data"])], "piece": a_csr + [count]}[which]
    if which == "assemble":
        return Entry([Input("cn", count, count + 1)], call, want, prepare=prepare, finish=finish)
    return Entry([], call, {"real": want(None), "decoy": None}, outs=outs, prepare=prepare, finish=finish)


def _bumped(entries):
    """Exported table entries with every count one more (an entry: {u64 hash, u64 reserved, u32 count | u32 ~first << 32, u32 off | u32 n
    << 32}: test_gpu_caller_views.py): another valid table over the same keys."""
    out = entries.clone()
    out.view(-1, 4)[:, 2] += 1
    return out


def _tables_entry(stage):
    """The one-card rehearsal of test_gpu_dist.py with one shard: ``table_export_device`` -> ``table_merge_device`` on a handle of its own
    -> ``table_export_device`` -> ``table_adopt_device`` on the root, finalize, export == the C oracle.  ``stage``: which of the three is
    made while its tensors are in flight -- ``export``: the two outputs' fill is queued; ``merge`` / ``adopt``: the entries are late, the
    decoy the same table with every count one more (its answer: the oracle's with every EC counted once more)."""
    import torch
    t, T, H, exp = _short()

    def mk():
        return ecb.EcBuilder(T, H, ec_capacity=1 << 10, arena_capacity=1 << 24)

    def exported(b):
        ne, npairs, _ = b.table_sizes()
        ent, prs = torch.zeros(max(ne * 4, 1), dtype=torch.int64, device="cuda"), torch.zeros(max(npairs, 1), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        b.table_export_device(ent, prs, 0)
        torch.cuda.synchronize()
        return ent, ne, prs, npairs

    def prepare():
        shard, part, root = mk(), mk(), mk()                               # (made before anything is in flight: ecb_create waits for the device)
        shard.push(*(t[k] for k in STREAMS))
        state = {"shard": shard, "part": part, "root": root, "handles": [shard, part, root], "counters": shard.counters()}
        if stage == "export":
            ne, npairs, _ = shard.table_sizes()
            state.update(ne=ne, npairs=npairs, outs=[("ent", (max(ne * 4, 1),), np.int64), ("prs", (max(npairs, 1),), np.int64)])
            return state
        tab = exported(shard)
        if stage == "adopt":
            part.table_merge_device(*tab)
            tab = exported(part)
        state.update(tab=tab, inputs=[Input("ent", tab[0], _bumped(tab[0])), Input("prs", tab[2])])
        return state

    def rest(state, tab, merged):
        """From a table on: merged on a handle of its own and exported unless it has been, adopted by the root, finalized, exported."""
        if not merged:
            state["part"].table_merge_device(*tab)
            tab = exported(state["part"])
        state["root"].table_adopt_device(*tab)
        return state["root"]

    def call(v, state):
        if stage == "export":
            state["shard"].table_export_device(v["ent"], v["prs"], 0)
            return [v["ent"], v["prs"]]
        _, ne, _, npairs = state["tab"]
        if stage == "merge":
            state["part"].table_merge_device(v["ent"], ne, v["prs"], npairs)
            return state["part"]
        state["root"].table_adopt_device(v["ent"], ne, v["prs"], npairs)
        return state["root"]

    def finish(out, state):
        try:
            if stage == "export":
                root = rest(state, (out[0], state["ne"], out[1], state["npairs"]), False)
            elif stage == "merge":
                root = rest(state, exported(out), True)
            else:
                root = out
            root.add_counters(*state["counters"])
            return _exported(root)
        finally:
            for b in state["handles"]:
                b.close()
    real = _oracle(t, H)
    bumped = list(real)
    bumped[5] = real[5] + 1
    return Entry([], call, {"real": real, "decoy": bumped if stage != "export" else None}, prepare=prepare, finish=finish)


def _triples_entry(stage):
    """The multisample protocol with one shard (test_gpu_multisample.py::_sharded): ``ms_local_triples_device`` into outputs whose fill is
    queued (``local``), ``ms_adopt_triples_device`` from counts that are late (``adopt``; the decoy: every count one more) == the
    triples of one handle over the stream."""
    import torch
    import test_gpu_multisample as tm
    st = _cached("ms_stream", lambda: tm._random_stream(np.random.default_rng(48), np.arange(300) * 5, 6000, 4, n_tpl=500))
    tr = _cached("ms_expected", st.expected)[0]

    def mk(ms):
        return ecb.EcBuilder(st.n_loci, tm.H, ec_capacity=1 << 12, multisample=ms)

    def dev(n, dt):
        return torch.zeros(max(int(n), 1), dtype=dt, device="cuda")

    def prepare():
        shard, part, root = mk(True), mk(False), mk(True)
        state = {"handles": [shard, part, root], "shard": shard, "root": root}
        shard.push(st.read_id, st.locus, st.hapflag)
        shard.push_cells(st.meta, 0)
        ne, npairs, nreads = shard.table_sizes()
        ent, prs = dev(ne * 4, torch.int64), dev(npairs, torch.int64)
        torch.cuda.synchronize()
        shard.table_export_device(ent, prs, 0)
        part.table_merge_device(ent, ne, prs, npairs)
        pe_n, pp_n, _ = part.table_sizes()
        pe, pp = dev(pe_n * 4, torch.int64), dev(pp_n, torch.int64)
        torch.cuda.synchronize()
        part.table_export_device(pe, pp, 0)
        root.table_adopt_device(pe, pe_n, pp, pp_n)
        a, v, _ = shard.counters()
        root.add_counters(a, v, nreads)
        s = root.finalize()
        E, nnz = s["n_ecs"], s["nnz_a"]
        keys, ip, ix, da = dev(E, torch.int64), dev(E + 1, torch.int32), dev(nnz, torch.int32), dev(nnz, torch.int32)
        torch.cuda.synchronize()
        root.export_ec_keys_device(keys)
        root.export_device(ip, ix, da)
        torch.cuda.synchronize()
        state.update(csr=(keys, ip, ix, da, E), nreads=nreads)
        if stage == "local":
            state["outs"] = [("key", (nreads,), np.int64), ("cnt", (nreads,), np.int32), ("first", (nreads,), np.int32)]
            return state
        key, cnt, first = dev(nreads, torch.int64), dev(nreads, torch.int32), dev(nreads, torch.int32)
        torch.cuda.synchronize()
        n = shard.ms_local_triples_device(keys, ip, ix, da, E, 0, key, cnt, first)
        torch.cuda.synchronize()
        state.update(n=n, inputs=[Input("key", key), Input("cnt", cnt, cnt + 1), Input("first", first)])
        return state

    def call(v, state):
        if stage == "local":
            keys, ip, ix, da, E = state["csr"]
            state["n"] = state["shard"].ms_local_triples_device(keys, ip, ix, da, E, 0, v["key"], v["cnt"], v["first"])
            return [v["key"], v["cnt"], v["first"]]
        state["root"].ms_adopt_triples_device([(v["key"], v["cnt"], v["first"], state["n"])])
        return []

    def finish(out, state):
        try:
            if stage == "local":
                state["root"].ms_adopt_triples_device([(out[0], out[1], out[2], state["n"])])
            got = state["root"].export_pairs()
            return [got[k] for k in ("ec", "cell", "file", "count", "first")]
        finally:
            for b in state["handles"]:
                b.close()
    real = [tr[k] for k in ("ec", "cell", "file", "count", "first")]
    bumped = list(real)
    bumped[3] = real[3] + 1
    return Entry([], call, {"real": real, "decoy": bumped if stage != "local" else None}, prepare=prepare, finish=finish)


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
ALL3 = ("i64", "strided", "cpu")
#: entry point -> (its Entry, the conversions the wrapper can be made to queue for it)
WRAPPERS = {
    "csr_to_hapcsc": (entry_csr_to_hapcsc, ALL3), "csr_to_hapcsc_values": (entry_csr_to_hapcsc_values, ALL3),
    "hapcsc_to_csr": (entry_hapcsc_to_csr, ALL3), "apply_mask": (entry_apply_mask, ALL3), "count_alignments": (entry_count_alignments, ALL3),
    "quantify": (entry_quantify, ALL3), "quantify_model": (entry_quantify_model, ALL3), "posterior": (entry_posterior, ALL3),
    "cell_support": (entry_cell_support, ALL3), "quantify_cells": (entry_quantify_cells, ALL3),
    "quantify_cells_model": (entry_quantify_cells_model, ALL3), "combine": (entry_combine, ALL3), "bundle": (entry_bundle, ALL3),
    "select": (entry_select, ALL3), "salmon_ecs": (entry_salmon_ecs, ("strided",)),     # (one tensor, of bytes; the ids are host arrays)
    "resample": (entry_resample, ALL3), "quantify_bootstrap": (entry_quantify_bootstrap, ALL3), "components": (entry_components, ALL3),
    "bus_molecules": (entry_bus_molecules, ALL3), "bus_correct": (entry_bus_correct, ("strided", "cpu")),      # (bytes and 64-bit words)
    "best_strata": (entry_best_strata, ALL3), "best_strata_inplace": (entry_best_strata_inplace, ("i64", "strided")),   # (only the scores convert)
    "collapse_umis": (entry_collapse_umis, ALL3),
}
HANDLE = dict([("push_device-" + c, (lambda c=c: _push("device", c))) for c in ("std", "par", "short", "std_hinted")], **{
    "push_device_tiled": lambda: _push("tiled"), "verify_device": entry_verify_device, "push_cells_device": entry_push_cells_device,
    "export_device": lambda: _export("csr"), "export_ec_keys_device": lambda: _export("keys"), "export_piece_device": lambda: _export("piece"),
    "assemble_ranges_device": lambda: _export("assemble"),
    "table_export_device": lambda: _tables_entry("export"), "table_merge_device": lambda: _tables_entry("merge"),
    "table_adopt_device": lambda: _tables_entry("adopt"), "ms_local_triples_device": lambda: _triples_entry("local"),
    "ms_adopt_triples_device": lambda: _triples_entry("adopt")})
CASES = [(name, mode) for name, (_, conv) in WRAPPERS.items() for mode in fl.MODES
         if "converted" not in mode or mode.rsplit("-", 1)[1] in conv]
CASES += [(name, mode) for name in HANDLE for mode in ("off", "default-late", "side-late")]


def _entry(name):
    return _cached(("entry", name), WRAPPERS[name][0] if name in WRAPPERS else HANDLE[name])


def run_case(name, mode, monkeypatch=None, record=None):
    """One case; ``record``: a dict that receives what happened (``tests`` pass none: they assert)."""
    import torch
    import test_gpu_thresholds as th
    e = _entry(name)
    fl.cycles_per_ms()                                                      # (calibrated before anything is in flight)
    if monkeypatch is not None:
        th._force(monkeypatch, e.env)
    state = e.prepare()
    inputs = state.get("inputs", e.inputs) if isinstance(state, dict) else e.inputs
    outs = state.get("outs", e.outs) if isinstance(state, dict) else e.outs
    # the decoy's own answer differs from the real one, on the checker, on the CPU: no case is vacuous
    if isinstance(e.want, dict):
        want, want_decoy = e.want["real"], e.want["decoy"]
    else:
        fl.check_rule(inputs)
        want, want_decoy = _cached(("want", name), lambda: (e.want({i.name: i.real for i in inputs}), e.want({i.name: i.decoy for i in inputs})))
    if want_decoy is None:
        assert outs and not inputs           # (only outputs are late: a fill that lands on the result leaves no answer at all)
    else:
        assert not fl.same(want_decoy, want), "the decoy's answer is the real one"
    finished = None if record is not None else _finished(name, monkeypatch)      # (first, so that no first-use cost falls into the delay)
    where, _, how = mode.partition("-")
    late = fl.Late(inputs, how.rsplit("-", 1)[1] if how.startswith("converted") else None, outs)
    stream = torch.cuda.Stream() if where == "side" else torch.cuda.current_stream()
    assert (stream != torch.cuda.default_stream()) == (where == "side")
    with torch.cuda.stream(stream):
        if where == "off":
            late.settle()
        else:
            late.arm(stream)
            assert late.converted == how.startswith("converted")
            assert late.in_flight()                                         # the producer is in flight on the line before the call
        t0 = time.perf_counter()
        out = e.call(late.v, state)
        call_ms = (time.perf_counter() - t0) * 1e3
        in_flight_after = where != "off" and late.in_flight()
        cloned, fills = fl.reuse_after(out, late)
        result = e.finish(cloned, state)
        torch.cuda.synchronize()
    got, still = fl.flat(result), fl.flat(out)
    if record is not None:
        record.update(checker=(fl.same(got[:len(want)], want) if e.exact else None), decoy=(e.exact and want_decoy is not None and
                                                                                            fl.same(got[:len(want_decoy)], want_decoy)),
                      got=got, in_flight_after=in_flight_after, call_ms=call_ms)
        return record
    if e.exact:
        assert fl.same(got[:len(want)], want), "the result is not the checker's" + (
            ": it is the decoy's" if want_decoy is not None and fl.same(got[:len(want_decoy)], want_decoy) else "")
    assert fl.same(got, finished), "the result is not that of the same call on finished tensors"
    if e.plain and not name.endswith("inplace"):
        assert fl.same(still, got), "an output changed after the call returned"
    del fills


def _finished(name, monkeypatch):
    """The same call on finished tensors, on the default stream, once per entry point."""
    return _cached(("finished", name), lambda: run_case(name, "off", monkeypatch, record={})["got"])


@pytest.mark.parametrize("name,mode", CASES, ids=["%s-%s" % c for c in CASES])
def test_tensors_in_flight_on_the_current_stream(name, mode, monkeypatch):
    run_case(name, mode, monkeypatch)


def test_the_delay_outlasts_what_it_has_to():
    """The calibrated delay is what the helper's docstring says, within the calibration's own precision: a sleep of DELAY_MS between two
    events takes at least nine tenths of it."""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fl.cycles_per_ms()
    a.record()
    fl.delay()
    b.record()
    b.synchronize()
    assert fl.DELAY_MS == fl.FACTOR * fl.CALL_MS and a.elapsed_time(b) >= 0.9 * fl.DELAY_MS, a.elapsed_time(b)
