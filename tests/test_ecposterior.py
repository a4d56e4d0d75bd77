"""ecquant's posterior without a GPU: the checker (tests/post_checker.py) pinned to the arrays recorded from the reference
(``tests/golden/post_cases.json``: what its ``multiply`` / ``normalize_reads`` leave in the matrix before ``sum(axis=READ)``), the rows'
sums, the weighted sum against the recorded next theta, the permutation between bit order and EMASE's layout, the constants and the header,
the ``.h5`` round trip of the values, and the command's wiring.

The tolerances are derived, not measured.  Every term is non-negative, so nothing cancels, and a value carries one rounding of 2^-53 per
addition in the longest chain of each sum it depends on, plus one per multiplication and division.  With B = the most set bits in a row,
M = the most members of a gene, H haplotypes (Phi_gh has M terms, Phi_g M H, Phi_t H) and R = the most genes in a row -- the terms of
``test_ecquant_models.py``, whose chains these are with the weight replaced by 1 and without the column sum (its L - 1 additions), since
the posterior is not summed over rows:

  model 4   phi (1) -> d[e] (B - 1 more: B in all) -> phi / d (1):                                                      B + 2
  the gene factor      phi (1) -> Phi_g (M H) -> the gene denominator (R - 1 more) -> 1 / it (1) -> x Phi_g (1 + M H):   R + 2 M H + 1
  model 3   / D (1 + B), x phi (1 + 1):                                                                                 B + R + 2 M H + 4
  model 1   Phi_gh / D_h (1 + M + B), / the allele denominator (1 + H - 1 + M), x the gene factor (1), x phi (2):       B + R + 2 M H + 2 M + H + 5
  model 2   Phi_t / the isoform denominator (1 + H + M - 1 + H), x the gene factor (1), / D_t (1 + H), x phi (2):        R + 2 M H + M + 3 H + 5

roundings on either side; two evaluations agree when they differ by at most that many plus the customary 2, times 2^-52, of the
reference's value, entry by entry, with exactly the same entries 0.  For models 1-3 that is one more than the chain asks: the bound is
``Grouping.tolerance``'s without its L term, as it stands there, and never above the bound of the step (``post_checker.tolerance``).
A reciprocal in place of a division is one more rounding and stays within the customary 2.

A row's values sum to 1: the quotients phi_i / d share d's error, so the sum is off by d's (B - 1) roundings, the quotients' one and
the B - 1 of the sum itself: within B 2^-52.

The checker against the reference's recorded arrays, worst relative difference and bound per case (all models and both thetas):
c1 4.6e-16 of 3.11e-15, ms 3.7e-16 of 1.78e-15, c1_len 5.2e-16 of 3.11e-15, h8 3.8e-15 of 1.71e-13 (each the smallest bound of its models)."""
import os
import re
import subprocess

import numpy as np
import pytest

from alntools_amd import bin_utils, ecb, emase_h5

import post_checker as pchk
import quant_checker as qchk
import quant_model_checker as mchk

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = pchk.GOLDEN


@pytest.fixture(autouse=True)
def _logger_level_as_it_was():
    import logging
    log = logging.getLogger("alntools.utils")
    level = log.level
    yield
    log.setLevel(level)


def _checker(case, model, k):
    r = pchk.load_case(case)
    key = ("checker", case["name"], model, k)
    if key not in pchk._loaded:                   # (computed once, shared by the tests below, never changed)
        pchk._loaded[key] = pchk.posterior(r.grouping(model), r.lay, model, r.theta[(model, k)], r.scale)
    return r, pchk._loaded[key][0], pchk._loaded[key][1]


def test_the_recorded_cases_are_the_ones_the_issue_names():
    assert [(c["name"], c["ec"], c["use_lengths"], c["models"], c["steps"], c["subset"]) for c in pchk.CASES] == [
        ("c1", "g2_c1.bin", False, [4, 1, 2, 3], [0, 5], False), ("ms", "g4b_multi_min0.bin", False, [4, 1, 2, 3], [0, 5], False),
        ("c1_len", "g2_c1.bin", True, [4], [0, 5], False), ("h8", "gt_h8_in.bin", False, [4, 1, 2, 3], [0, 5], True)]
    for c in pchk.CASES:
        for f in c["npz"]:
            assert os.path.getsize(os.path.join(GOLDEN, f)) <= 970265
    # h8 records its row of 3 598 set bits, the 200 rows after it and every 10th row
    r = pchk.load_case(pchk.CASES[3])
    bits = np.bincount(r.lay.bit_row, minlength=r.lay.E)
    big = int(np.argmax(bits))
    assert bits[big] == 3598 == r.case["B"]
    assert np.array_equal(r.rows, np.unique(np.concatenate([np.arange(big, min(r.lay.E, big + 201)), np.arange(0, r.lay.E, 10)])))
    assert all(pchk.load_case(c).rows is None for c in pchk.CASES[:3])


@pytest.mark.parametrize("case", pchk.CASES, ids=lambda c: c["name"])
def test_the_checker_sees_the_recorded_shapes_and_sum_lengths(case):
    r = pchk.load_case(case)
    assert list(r.m.shape) == case["shape"] and (r.p.B, r.p.L) == (case["B"], case["L"])
    if case["grp"] is not None:
        assert (r.q.M, r.q.R) == (case["M"], case["R"])
    assert r.lay.n_bits == len(r.p.bit_flat) and np.array_equal(np.sort(r.lay.hm_to_bit), np.arange(r.lay.n_bits))
    for key, ref in r.ref.items():
        assert ref.shape == (int(r.kept.sum()),) and ref.dtype == np.float64, key


@pytest.mark.parametrize("case,model,k", pchk.TRIPLES, ids=pchk.TRIPLE_IDS)
def test_the_checker_reproduces_every_recorded_posterior(case, model, k):
    r, post, mass = _checker(case, model, k)
    bound = r.bound(model)
    worst = qchk.agree(r.recorded_of(post), r.ref[(model, k)], bound)
    print("%s model %d k=%d: worst relative difference %.3g, bound %.3g" % (case["name"], model, k, worst, bound))
    assert bound <= r.step_bound(model)                                     # never above the bound of the step


@pytest.mark.parametrize("case,model,k", pchk.TRIPLES, ids=pchk.TRIPLE_IDS)
def test_every_row_of_the_checker_sums_to_1_or_is_exactly_0(case, model, k):
    r, post, mass = _checker(case, model, k)
    sums = np.bincount(r.lay.bit_row, weights=post, minlength=r.lay.E)
    live = mass > 0
    worst = float(np.abs(sums[live] - 1.0).max())
    print("%s model %d k=%d: a row's sum is off 1 by at most %.3g, bound %.3g" % (case["name"], model, k, worst, case["B"] * 2.0 ** -52))
    assert worst <= case["B"] * 2.0 ** -52
    assert not post[~live[r.lay.bit_row]].any() and np.all(post >= 0)


@pytest.mark.parametrize("case,model,k", pchk.TRIPLES, ids=pchk.TRIPLE_IDS)
def test_the_weighted_sum_of_the_posterior_is_the_recorded_next_theta(case, model, k):
    r, post, mass = _checker(case, model, k)
    worst = qchk.agree(pchk.weighted_sum(r.p, r.lay, post), r.next[(model, k)], r.step_bound(model))
    print("%s model %d k=%d: worst relative difference %.3g, bound %.3g" % (case["name"], model, k, worst, r.step_bound(model)))
    # ... and bit for bit the checkers' own step, whose weighted sum this is
    own = qchk.step(r.p, r.theta[(model, k)], r.scale)[0] if model == 4 else mchk.step(r.q, model, r.theta[(model, k)], r.scale)[0]
    qchk.agree(pchk.weighted_sum(r.p, r.lay, post), own, r.step_bound(model))


def test_a_row_nothing_explains_is_all_0_and_row_mass_says_so():
    # H = 2, three rows; theta = 0 on both targets of row 1
    p = qchk.Problem([0, 2, 4, 5], [0, 2, 1, 3, 2], [3, 1, 3, 2, 0], 4, 2, [0, 3], [0, 1, 2], [4, 0, 2])
    lay = pchk.Layout([0, 2, 4, 5], [0, 2, 1, 3, 2], [3, 1, 3, 2, 0], 4, 2)
    theta = np.array([[1.0, 0.0, 3.0, 0.0], [2.0, 0.0, 0.5, 0.0]])
    q = mchk.Grouping(p, [0, 0, 1, 1], 2)
    assert lay.bit_ptr.tolist() == [0, 2, 3, 5, 6, 6] and lay.n_bits == 6     # (the stored mask of 0 has no bits)
    for model in (4, 1, 2, 3):
        post, mass = pchk.posterior(q, lay, model, theta)
        assert mass.tolist() == [6.0, 0.0, 0.0] and not post[3:].any() and abs(post[:3].sum() - 1.0) < 1e-15
    post, _ = pchk.posterior(p, lay, 4, theta)
    assert post.tolist() == [1.0 / 6.0, 2.0 / 6.0, 3.0 / 6.0, 0.0, 0.0, 0.0]  # bit order: non-zero (0, t0) bits 0 and 1, then (0, t2) bit 0


@pytest.mark.parametrize("case", pchk.CASES, ids=lambda c: c["name"])
def test_the_permutation_between_bit_order_and_the_emase_layout_is_an_exact_inverse(case):
    r = pchk.load_case(case)
    lay, m = r.lay, r.m
    payload = np.arange(lay.n_bits, dtype=np.float64) * 3.0 + 1.0
    csc = lay.to_csc(payload)
    assert np.array_equal(lay.from_csc(csc), payload) and np.array_equal(np.sort(lay.csc_to_bit), np.arange(lay.n_bits))
    assert np.array_equal(lay.to_csc(lay.from_csc(payload)), payload)
    # the layout is scipy's: haplotype h's block is the csc of its incidence, and the payload lands at the entry it belongs to
    row = np.repeat(np.arange(lay.E), np.diff(m.indptrA))
    start = 0
    for h in range(lay.H):
        ref = m.haplotype_csc(h)
        n = ref.nnz
        assert np.array_equal(lay.csc_indptr[h], ref.indptr) and np.array_equal(lay.csc_indices[start:start + n], ref.indices)
        has = np.flatnonzero((m.dataA >> h) & 1)
        at = lay.bit_ptr[has] + np.array([bin(int(x) & ((1 << h) - 1)).count("1") for x in m.dataA[has]], dtype=np.int64)
        from scipy.sparse import csr_matrix
        want = csr_matrix((payload[at], (row[has], m.indicesA[has])), shape=(lay.E, lay.T)).tocsc()
        assert np.array_equal(csc[start:start + n], want.data)
        start += n
    assert start == lay.n_bits


# ---- the constants and the ABI --------------------------------------------------------------------------------------------------------------
def test_the_constants_the_new_kernels_share_are_the_ones_the_tests_straddle_and_no_float_atomics_are_added():
    from test_quant_constants import Q_LONG_ROW
    from test_ecquant_models import Q_LONG_GENE
    csrc = os.path.join(ROOT, "alntools_amd", "csrc")
    src = open(os.path.join(csrc, "quant_post.inc")).read()
    assert not re.findall(r"constexpr\s+u32\s+Q_\w+", src)                  # it defines no threshold of its own ...
    assert [d.strip() for d in re.findall(r"constexpr\s+u32\s+Q_LONG_ROW\s*=\s*([^;,]+);", open(os.path.join(csrc, "quant.inc")).read())] == [str(Q_LONG_ROW)]
    assert [d.strip() for d in re.findall(r"constexpr\s+u32\s+Q_LONG_GENE\s*=\s*([^;,]+);", open(os.path.join(csrc, "quant_model.inc")).read())] == [str(Q_LONG_GENE)]
    # ... and branches on the shared ones where the row pass does: short rows by a lane through the tile, long rows by a workgroup
    assert len(re.findall(r"b - a <= Q_LONG_ROW", src)) == 1 and len(re.findall(r"> Q_LONG_ROW\)", src)) == 1 and "v[Q_TILE]" in src
    # (the long genes and long rows of the chain: quant_model.inc's qm_step, which this file runs once; the long rows' sum: quant.inc's q_long_row_sum)
    model, flat = (open(os.path.join(csrc, f)).read() for f in ("quant_model.inc", "quant.inc"))
    step = model.split("void qm_step(")[1].split("\n}\n")[0]
    assert len(re.findall(r"\bqm_step\(", src)) == 1 and len(re.findall(r"k_qm_ghlong<<<", step)) == 1 and len(re.findall(r"k_qm_rowlong<<<", step)) == 1
    assert len(re.findall(r"k_qm_ghlong<<<", model)) == 1 and len(re.findall(r"k_qm_rowlong<<<", model)) == 1
    assert "q_long_row_sum(s, " in src and "q_block_sum" in flat.split("double q_long_row_sum(")[1].split("\n}\n")[0]
    assert [d.strip() for d in re.findall(r"QP_ERR_THETA\s*=\s*([^ ,}]+)", src)] == ["8u"]            # beside Q_ERR_SCALE 1, Q_ERR_THETA 2, Q_ERR_GENE 4
    for text in (src, open(os.path.join(csrc, "ecb.hip")).read().split("k_cvv_bits")[1].split("k_iota")[0]):
        assert "atomicAdd(reinterpret_cast<double" not in text and "unsafeAtomicAdd" not in text and "hipGraph" not in text and not re.search(r"\basm\b", text)
    hip = open(os.path.join(csrc, "ecb.hip")).read()
    assert len(re.findall(r'^#include "quant_post\.inc"', hip, re.M)) == 1


def test_the_abi_declares_the_four_entries_in_a_header_of_their_own():
    hdr = open(os.path.join(ROOT, "include", "ecb_quant_post.h")).read()
    quant = open(os.path.join(ROOT, "include", "ecb_quant.h")).read()
    main = open(os.path.join(ROOT, "include", "ecb.h")).read()
    assert ecb.QUANT_POST_SYMBOLS == ("ecb_posterior_device", "ecb_posterior", "ecb_csr_to_hapcsc_values_device", "ecb_csr_to_hapcsc_values")
    assert sorted(set(re.findall(r"^int (ecb_\w+)\(", hdr, re.M))) == sorted(ecb.QUANT_POST_SYMBOLS)
    assert len(re.findall(r'^#include "ecb_quant_post\.h"', quant, re.M)) == 1 and "ECB_ABI_VERSION 4" in main and ecb.ABI_VERSION == 4
    assert not set(ecb.QUANT_POST_SYMBOLS) & (set(ecb.SYMBOLS) | set(ecb.COUNT_SYMBOLS) | set(ecb.BUNDLE_SYMBOLS) | set(ecb.SELECT_SYMBOLS)
                                              | set(ecb.QUANT_SYMBOLS) | set(ecb.QUANT_MODEL_SYMBOLS) | set(ecb.QUANT_CELLS_SYMBOLS)
                                              | set(ecb.QUANT_CELLS_MODEL_SYMBOLS))
    from alntools_amd import build
    assert any(p.endswith("ecb_quant_post.h") for p in build.inputs()) and any(p.endswith("quant_post.inc") for p in build.inputs())
    # a C compiler sees them through ecb.h alone
    src = ('#include "ecb.h"\n'
           "int (*a)(int, uint32_t, uint32_t, uint32_t, uint64_t, const int32_t*, const int32_t*, const int32_t*, const double*, const double*, uint32_t, "
           "const int32_t*, uint32_t, uint64_t, double*, int64_t*, double*) = ecb_posterior;\n"
           "int (*b)(int, uint32_t, uint32_t, uint32_t, uint64_t, const void*, const void*, const void*, const void*, const void*, uint32_t, "
           "const void*, uint32_t, uint64_t, void*, void*, void*) = ecb_posterior_device;\n"
           "int (*c)(int, uint32_t, uint32_t, uint32_t, const int32_t*, const int32_t*, const int32_t*, const double*, int32_t*, int32_t*, double*, "
           "uint64_t, uint64_t*) = ecb_csr_to_hapcsc_values;\n"
           "int (*d)(int, uint32_t, uint32_t, uint32_t, const void*, const void*, const void*, const void*, void*, void*, void*, uint64_t*) = "
           "ecb_csr_to_hapcsc_values_device;\n")
    r = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the library exports them
    lib = ecb.load()
    for s in ecb.QUANT_POST_SYMBOLS:
        assert hasattr(lib, s), s


# ---- the .h5 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c1", "ms"])
def test_values_round_trip_through_the_h5_bit_for_bit(tmp_path, name):
    """Through whichever backend ``emase_h5`` finds (libhdf5 itself where neither PyTables nor h5py is installed)."""
    case = [c for c in pchk.CASES if c["name"] == name][0]
    r, post, mass = _checker(case, 4, 5)
    post = post.copy()
    post[::7] = 0.0                                                          # explicit zeros are stored: the file's incidence stays A's
    f = str(tmp_path / "p.h5")
    emase_h5.save(f, r.m, incidence_only=False, hapcsc=r.lay.hapcsc(post))
    got = emase_h5.load_values(f)
    want = r.lay.to_csc(post)
    start = 0
    for h, (ip, ix, data) in enumerate(got):
        n = len(ix)
        assert np.array_equal(ip, r.lay.csc_indptr[h]) and np.array_equal(ix, r.lay.csc_indices[start:start + n])
        assert data.dtype == np.float64 and data.tobytes() == want[start:start + n].tobytes()
        start += n
    assert len(got) == r.m.num_haplotypes and start == r.lay.n_bits
    back = emase_h5.load(f, csr=emase_h5.scipy_csr)                          # the incidence, zeros and all: the .bin's A
    assert np.array_equal(back.indptrA, r.m.indptrA) and np.array_equal(back.indicesA, r.m.indicesA) and np.array_equal(back.dataA, r.m.dataA)
    assert np.array_equal(back.dataN, r.m.dataN) and back.lname == r.m.lname and back.sname == r.m.sname
    # incidence_only=True writes no data
    emase_h5.save(f, r.m, incidence_only=True, hapcsc=r.lay.hapcsc(post))
    with pytest.raises(Exception):
        emase_h5.load_values(f)


# ---- the command ------------------------------------------------------------------------------------------------------------------------------
def test_the_command_line_hands_the_posterior_file_to_methods(tmp_path, monkeypatch):
    from click.testing import CliRunner
    from alntools_amd import cli, methods
    e = tmp_path / "e.bin"
    e.write_bytes(b"")
    g = tmp_path / "g.txt"
    g.write_text("")
    o, w = str(tmp_path / "o.tsv"), str(tmp_path / "o.h5")
    seen = []
    monkeypatch.setattr(methods, "ecquant", lambda *a, **kw: seen.append((a, kw)))
    for argv in (["-w", w], ["--posterior", w, "-M", "2", "-g", str(g), "-l", "-s", "x"], []):
        r = CliRunner().invoke(cli.cli, ["ecquant", str(e), o] + argv)
        assert r.exit_code == 0, r.output
    assert seen == [((str(e), o, None, False, 1000, 1e-6), {"posterior_file": w}),
                    ((str(e), o, "x", True, 1000, 1e-6, 2, str(g)), {"posterior_file": w}), ((str(e), o, None, False, 1000, 1e-6), {})]
    assert "--posterior" in CliRunner().invoke(cli.cli, ["ecquant", "--help"]).output
    assert "ecquant sample.bin abundances.tsv -w posterior.h5" in open(os.path.join(ROOT, "README.md")).read() and "``-w``" in cli.__doc__
    # methods hands it on by name, and only when it is given
    calls = []
    monkeypatch.undo()
    monkeypatch.setattr(bin_utils, "ecquant", lambda *a, **kw: calls.append(kw))
    methods.ecquant("a", "b", posterior_file="c")
    methods.ecquant("a", "b")
    assert calls[0]["posterior_file"] == "c" and "posterior_file" not in calls[1]


def _fake_quantify(indptr, indices, data, n_loci, n_haps, indptr_n, indices_n, data_n, sample=None, scale=None, theta_in=None, max_iters=1000, tol=1e-6,
                   device=0):
    return qchk.run(qchk.Problem(indptr, indices, data, n_loci, n_haps, indptr_n, indices_n, data_n, sample), scale, theta_in, max_iters, tol)


def _fake_posterior(indptr, indices, data, n_loci, n_haps, theta, scale=None, gene=None, n_genes=0, model=4, device=0):
    lay = pchk.Layout(indptr, indices, data, n_loci, n_haps)
    p = qchk.Problem(indptr, indices, data, n_loci, n_haps, [0, 0], [], [])
    post, mass = pchk.posterior(p if model == 4 else mchk.Grouping(p, gene, n_genes), lay, model, theta, scale)
    return post, lay.bit_ptr, mass


def test_ecquant_with_the_checkers_as_the_device_writes_both_files_or_neither(tmp_path, monkeypatch, caplog):
    monkeypatch.setattr(ecb, "quantify", _fake_quantify)
    monkeypatch.setattr(ecb, "posterior", _fake_posterior)
    case = pchk.CASES[0]
    r = pchk.load_case(case)
    src, out, h5 = os.path.join(GOLDEN, case["ec"]), str(tmp_path / "o.tsv"), str(tmp_path / "o.h5")
    factory = lambda post: r.lay.hapcsc(post)                                # noqa: E731
    bin_utils.ecquant(src, out, max_iters=3, tol=0.0, posterior_file=h5, hapcsc=factory)
    theta, _ = qchk.run(r.p, max_iters=3, tol=0.0)
    assert open(out).read() == bin_utils.quant_table(r.m.lname, r.m.hname, theta)
    want = r.lay.to_csc(pchk.posterior(r.p, r.lay, 4, theta)[0])              # the posterior at the RETURNED theta
    assert np.concatenate([d for _, _, d in emase_h5.load_values(h5)]).tobytes() == want.tobytes()
    os.remove(out); os.remove(h5)
    # a failing run leaves no file: an unknown sample (before the EM), and a table that cannot be written (after the .h5 has been)
    with pytest.raises(KeyError):
        bin_utils.ecquant(src, out, sample="nobody", posterior_file=h5, hapcsc=factory)
    assert not os.path.exists(out) and not os.path.exists(h5)
    with caplog.at_level("ERROR", logger="alntools.utils"):
        with pytest.raises(OSError):
            bin_utils.ecquant(src, str(tmp_path / "no" / "such" / "dir" / "o.tsv"), max_iters=1, tol=0.0, posterior_file=h5, hapcsc=factory)
    assert not os.path.exists(h5) and "Error:" in caplog.text
    with pytest.raises(Exception):
        bin_utils.ecquant(src, out, max_iters=1, tol=0.0, posterior_file=str(tmp_path / "no" / "such" / "dir" / "o.h5"), hapcsc=factory)
    assert not os.path.exists(out)
    # a file that was there before and that this run could not open is not this run's to remove; the table is not written either
    import stat
    if os.geteuid() != 0:                                                   # (root opens a read-only file for writing)
        with open(h5, "w") as fh:
            fh.write("an earlier run's")
        os.chmod(h5, stat.S_IRUSR)
        with pytest.raises(OSError):
            bin_utils.ecquant(src, out, max_iters=1, tol=0.0, posterior_file=h5, hapcsc=factory)
        assert open(h5).read() == "an earlier run's" and not os.path.exists(out)
        os.chmod(h5, stat.S_IRUSR | stat.S_IWUSR)
        os.remove(h5)
    old_dir = tmp_path / "o.tsv"                                              # the table's path is a directory: the .h5 goes, the directory stays
    old_dir.mkdir()
    with pytest.raises(OSError):
        bin_utils.ecquant(src, str(old_dir), max_iters=1, tol=0.0, posterior_file=h5, hapcsc=factory)
    assert not os.path.exists(h5) and old_dir.is_dir()
    old_dir.rmdir()
    # a keyword the function does not know is a TypeError, not ignored
    with pytest.raises(TypeError):
        bin_utils.ecquant(src, out, posterior_fil=h5)
    # -w through the command line with a failing run: exit 1, no file
    from click.testing import CliRunner
    from alntools_amd import cli
    res = CliRunner().invoke(cli.cli, ["ecquant", src, out, "-w", h5, "-s", "nobody"])
    assert res.exit_code == 1 and not os.path.exists(out) and not os.path.exists(h5)
