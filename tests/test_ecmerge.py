"""ecmerge without a GPU: the merge checker (tests/ec_merge_checker.py) pinned to the reference's bytes -- each golden alone, and g2's
stream cut into consecutive read ranges converted by the oracle -- ``bin_utils.plan_merge``, the command line's file list, and every
header refusal of the command (exit status 1, ``Error:``, no file written) before libecb is loaded."""
import os
import subprocess
import sys

import numpy as np
import pytest

from alntools_amd import bin_utils, ecb, synth
from oracle import ec_oracle as orc

import ec_merge_checker as chk

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDENS = ["g1_edge.bin", "g2_c1.bin", "g4_multi_min0.bin", "g4_multi_min20.bin", "g4_multi_min60.bin",
           "g4b_multi_min0.bin", "g4b_multi_min40.bin", "g4b_multi_min160.bin"]


def _bytes(p):
    with open(p, "rb") as f:
        return f.read()


@pytest.mark.parametrize("name", GOLDENS)
def test_the_checker_leaves_one_golden_unchanged(golden_dir, name):
    p = os.path.join(golden_dir, name)
    assert chk.merge_bytes([bin_utils.ecload(p)]) == _bytes(p)


@pytest.mark.parametrize("cuts", [[0, 5000, 10000], [0, 1, 3333, 6666, 9999, 10000], list(np.linspace(0, 10000, 8).astype(int))])
def test_the_checker_merges_g2_split_by_reads_into_the_whole(golden_dir, cuts):
    import json
    g = json.load(open(os.path.join(golden_dir, "g2_c1.json")))
    spec = synth.SynthSpec(**g["spec"])
    refs = spec.references()
    parts = []
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        out = orc.convert_records([r[0] for r in refs], [r[1] for r in refs], synth.raw_records(spec, int(r0), int(r1)), g["sample"])
        parts.append(bin_utils.ECMatrices(**_fields(orc.ecload_bytes(out["bin"]))))
    assert chk.merge_bytes(parts) == _bytes(os.path.join(golden_dir, "g2_c1.bin"))


def _fields(w):
    return dict(hname=w["hname"], lname=w["lname"], lengths=w["lengths"], sname=w["sname"], indptrA=w["indptrA"], indicesA=w["indicesA"],
                dataA=w["dataA"], indptrN=w["indptrN"], indicesN=w["indicesN"], dataN=w["dataN"])


def _m(lname, sname, hname=("A", "B"), lengths=None, rows=((0, 1),), counts=None):
    """A small ECMatrices: rows of (column, mask) pairs given as flat tuples (c0, m0, c1, m1, ...)."""
    lengths = np.arange(len(lname) * len(hname)).reshape(len(lname), len(hname)) + 100 if lengths is None else lengths
    ip = np.cumsum([0] + [len(r) // 2 for r in rows])
    ix = [r[i] for r in rows for i in range(0, len(r), 2)]
    dx = [r[i + 1] for r in rows for i in range(0, len(r), 2)]
    counts = counts if counts is not None else [[1] * len(rows) for _ in sname]
    ipn, ixn, dxn = [0], [], []
    for c in counts:
        nz = [e for e, v in enumerate(c) if v]
        ixn += nz
        dxn += [c[e] for e in nz]
        ipn.append(len(ixn))
    return bin_utils.ECMatrices(list(hname), list(lname), lengths, list(sname), ip, ix, dx, ipn, ixn, dxn)


def test_plan_of_identical_target_lists_maps_nothing():
    a, b = _m(["t0", "t1", "t0"], ["s"]), _m(["t0", "t1", "t0"], ["s", "u"])
    p = bin_utils.plan_merge([a, b])
    assert p.lname == ["t0", "t1", "t0"] and p.target_maps == [None, None]
    assert p.sname == ["s", "u"] and [m.tolist() for m in p.sample_maps] == [[0], [0, 1]]
    assert np.array_equal(p.lengths, np.asarray(a.lengths))


def test_plan_of_different_target_lists_is_the_union_in_first_seen_order():
    a = _m(["t0", "t1"], ["s"], lengths=np.array([[1, 2], [3, 4]]))
    b = _m(["t2", "t1", "t3"], ["u", "s"], lengths=np.array([[5, 6], [3, 4], [7, 8]]))
    p = bin_utils.plan_merge([a, b])
    assert p.lname == ["t0", "t1", "t2", "t3"]
    assert [m.tolist() for m in p.target_maps] == [[0, 1], [2, 1, 3]]
    assert p.lengths.tolist() == [[1, 2], [3, 4], [5, 6], [7, 8]]
    assert p.sname == ["s", "u"] and [m.tolist() for m in p.sample_maps] == [[0], [1, 0]]


@pytest.mark.parametrize("what", ["haplotypes", "lengths_same_lists", "lengths_union", "duplicate_target", "duplicate_sample", "empty"])
def test_plan_refusals(what):
    a = _m(["t0", "t1"], ["s"])
    b = {"haplotypes": _m(["t0", "t1"], ["s"], hname=("B", "A")),
         "lengths_same_lists": _m(["t0", "t1"], ["s"], lengths=np.array([[100, 101], [0, 103]])),
         "lengths_union": _m(["t1", "t2"], ["s"], lengths=np.array([[1, 1], [2, 2]])),
         "duplicate_target": _m(["t2", "t2"], ["s"]),
         "duplicate_sample": _m(["t0", "t1"], ["s", "s"], counts=[[1], [1]])}.get(what)
    with pytest.raises(ValueError):
        bin_utils.plan_merge([] if what == "empty" else [a, b])


def test_command_line_takes_the_inputs_then_the_directory_in_name_order(tmp_path, monkeypatch):
    from click.testing import CliRunner
    from alntools_amd import cli, methods
    d = tmp_path / "d"
    d.mkdir()
    for n in ("z.bin", "a.bin", "m.bin", "notes.txt"):
        (d / n).write_bytes(b"")
    i1, i2 = tmp_path / "y.bin", tmp_path / "b.bin"
    i1.write_bytes(b""); i2.write_bytes(b"")
    seen = []
    monkeypatch.setattr(methods, "ecmerge", lambda files, out: seen.append((list(files), out)))
    r = CliRunner().invoke(cli.cli, ["ecmerge", "-i", str(i1), "-i", str(i2), "-d", str(d), "-o", str(tmp_path / "o.bin")])
    assert r.exit_code == 0, r.output
    assert seen == [([str(i1), str(i2)] + [str(d / n) for n in ("a.bin", "m.bin", "z.bin")], str(tmp_path / "o.bin"))]


def _fake_combine(parts, n_loci, n_haps, n_samples, device=0):
    """ecb.combine through the checker: the maps name the columns and samples."""
    ms = []
    for p in parts:
        tm = p["target_map"] if p["target_map"] is not None else np.arange(p["n_loci"])
        lname = ["c%d" % c for c in tm]
        sname = ["s%d" % s for s in p["sample_map"]]
        ms.append(bin_utils.ECMatrices(["h"] * n_haps, lname, np.zeros((len(lname), n_haps)), sname, p["indptrA"], p["indicesA"], p["dataA"],
                                       p["indptrN"], p["indicesN"], p["dataN"]))
    m = chk.merge(ms)
    # (the checker numbers the columns and samples in first-seen order: back to the plan's numbers)
    cmap = np.array([int(t[1:]) for t in m.lname], dtype=np.int64)
    smap = np.array([int(s[1:]) for s in m.sname], dtype=np.int64)
    assert np.array_equal(cmap[np.argsort(cmap)], np.arange(n_loci))
    rows = [sorted(zip(cmap[m.indicesA[a:b]], m.dataA[a:b])) for a, b in zip(m.indptrA[:-1], m.indptrA[1:])]
    ip = np.cumsum([0] + [len(r) for r in rows])
    trip = sorted((smap[s], int(m.indicesN[q]), int(m.dataN[q])) for s in range(m.num_samples) for q in range(m.indptrN[s], m.indptrN[s + 1]))
    ipn = np.searchsorted(np.array([t[0] for t in trip], dtype=np.int64), np.arange(n_samples + 1))
    return (ip, [c for r in rows for c, _ in r], [d for r in rows for _, d in r], ipn, [t[1] for t in trip], [t[2] for t in trip])


def test_ecmerge_with_the_checker_as_the_device_writes_the_checkers_bytes(golden_dir, tmp_path, monkeypatch):
    monkeypatch.setattr(ecb, "combine", _fake_combine)
    rng = np.random.default_rng(3)
    a = chk.random_bin(rng, 300, ["t%d" % i for i in range(40)], ["A", "B", "C"], ["s1", "s2"], max_row=40)
    b = chk.random_bin(rng, 200, ["t%d" % i for i in range(30, 70)], ["A", "B", "C"], ["s2", "s3"], max_row=40)
    b.lengths[:10] = a.lengths[30:40]
    pa, pb, out = str(tmp_path / "a.bin"), str(tmp_path / "b.bin"), str(tmp_path / "o.bin")
    bin_utils.ecsave2(pa, a); bin_utils.ecsave2(pb, b)
    bin_utils.ecmerge([pa, pb], out)
    assert _bytes(out) == chk.merge_bytes([bin_utils.ecload(pa), bin_utils.ecload(pb)])
    g = os.path.join(golden_dir, "gt_ms.out.bin")
    bin_utils.ecmerge([g], out)
    assert _bytes(out) == chk.merge_bytes([bin_utils.ecload(g)])


def _run(args, tmp_path):
    env = dict(os.environ)
    env.pop("ALNTOOLS_GPUS", None)
    return subprocess.run([sys.executable, "-m", "alntools_amd.cli", "ecmerge"] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("what", ["haplotypes", "lengths", "duplicate_target", "no_inputs", "empty_directory"])
def test_command_line_refusals_exit_1_and_write_nothing(golden_dir, tmp_path, what):
    out = str(tmp_path / "out.bin")
    g1 = os.path.join(golden_dir, "g1_edge.bin")
    m = bin_utils.ecload(g1)
    p = str(tmp_path / "other.bin")
    if what == "haplotypes":
        m.hname = m.hname[::-1]
    elif what == "lengths":
        m.lengths = np.asarray(m.lengths) + 1
    elif what == "duplicate_target":
        m.lname = [m.lname[0]] * m.num_loci
    bin_utils.ecsave2(p, m)
    args = {"no_inputs": ["-o", out], "empty_directory": ["-d", str(tmp_path / "empty"), "-o", out]}.get(what, ["-i", g1, "-i", p, "-o", out])
    os.makedirs(str(tmp_path / "empty"))
    (tmp_path / "empty" / "readme.txt").write_text("x")
    r = _run(args, tmp_path)
    assert r.returncode == 1, r.stdout + r.stderr
    if what == "empty_directory":
        assert "No bin files found in directory: {}".format(tmp_path / "empty") in r.stdout
    else:
        assert "Error:" in r.stderr, r.stderr
        assert "libecb" not in r.stderr
    assert not os.path.exists(out)


def test_the_abi_declares_the_combine_entries():
    hdr = open(os.path.join(ROOT, "include", "ecb.h")).read()
    for s in ("ecb_combine_device", "ecb_combine"):
        assert s + "(" in hdr and s in ecb.SYMBOLS
    assert "ecb_combine_part" in hdr and ecb.ABI_VERSION == 4
