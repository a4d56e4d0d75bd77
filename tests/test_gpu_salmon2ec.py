"""salmon2ec on the GPU (``ecb_salmon_ecs`` / ``ecb_salmon_ecs_device``): every reference golden through the command line with the
reference's bytes and no PyTorch; the .gz input; seeded random directories and a config-3-sized one against the checker; every
refusal with its line number, each followed by a good call; the deviations from the reference, pinned."""
import gzip
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from alntools_amd import bin_utils, ecb, salmon_utils

import salmon_checker as chk

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _bytes(p):
    with open(p, "rb") as f:
        return f.read()


def _cases(golden_dir):
    return json.load(open(os.path.join(golden_dir, "salmon_cases.json")))


def _cli(args, importtime=False):
    env = dict(os.environ)
    env.pop("ALNTOOLS_TORCH", None)
    env.pop("ALNTOOLS_GPUS", None)
    pre = [sys.executable] + (["-X", "importtime"] if importtime else []) + ["-m", "alntools_amd.cli", "salmon2ec"]
    return subprocess.run(pre + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)


def _same(got, exp):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert np.array_equal(np.asarray(g, dtype=np.int64), np.asarray(e, dtype=np.int64))


def _good(n_targets=40):
    """A small good call and its expected arrays (checked after every refusal: the library must still work)."""
    rng = np.random.default_rng(n_targets)
    ptr, tid, counts = chk.random_ecs(rng, n_targets, 30)
    col, hap = np.arange(n_targets) // 2, np.arange(n_targets) % 2
    got = ecb.salmon_ecs(chk.ec_section(ptr, tid, counts), 30, col, hap, n_targets // 2, 2)
    ip, ix, da = chk.csr_from_targets(ptr, tid, col, hap, n_targets // 2)
    nz = np.flatnonzero(counts)
    _same(got, (ip, ix, da, nz, counts[nz]))


def test_every_golden_through_the_command_line_with_the_references_bytes(golden_dir, tmp_path):
    n = 0
    for c in _cases(golden_dir):
        if c["bin"] is None or c["name"].startswith("dev_"):
            continue
        out = str(tmp_path / (c["name"] + ".bin"))
        d = os.path.join(golden_dir, c["dir"])
        args = [d, out, "-s", c["sample"], "-v"] + (["-t", os.path.join(d, c["targets"])] if c["targets"] else [])
        r = _cli(args, importtime=True)
        assert r.returncode == 0, r.stderr[-2000:]
        imported = [l.split("|")[-1].strip() for l in r.stderr.splitlines() if l.startswith("import time:")]
        assert "alntools_amd.ecb" in imported
        assert not any(m == "torch" or m.startswith("torch.") for m in imported)
        assert "Error:" not in r.stderr
        assert _bytes(out) == _bytes(os.path.join(golden_dir, c["bin"])), c["name"]
        n += 1
    assert n == 7


def test_gz_input_gives_the_same_bytes(golden_dir, tmp_path):
    for name in ("diploid", "crlf", "long"):
        d = str(tmp_path / name)
        shutil.copytree(os.path.join(golden_dir, "salmon_" + name), d)
        p = os.path.join(d, "aux_info", "eq_classes.txt")
        with gzip.open(p + ".gz", "wb") as f:
            f.write(_bytes(p))
        os.remove(p)
        c = {c["name"]: c for c in _cases(golden_dir)}[name]
        out = str(tmp_path / (name + ".bin"))
        salmon_utils.convert(d, out, c["sample"])
        assert _bytes(out) == _bytes(os.path.join(golden_dir, c["bin"]))


@pytest.mark.parametrize("name,line,why", [
    ("dev_k", 10, "k differs from the number of target ids"),
    ("dev_repeat", 10, "a target id repeated within the line"),
    ("dev_fewer", 11, "the number of EC lines differs from the header's"),
    ("err_more_lines", 11, "the number of EC lines differs"),
    ("err_target_id", 10, "a target id at or beyond the number of targets"),
    ("err_letter", 10, "a byte other than a digit, tab or line end"),
    ("err_empty_line", 10, "an empty field"),
    ("err_empty_field", 10, "an empty field"),
    ("dev_quant_dup", 4, "target 'T1_B' is listed twice"),
    ("err_header_dup", 5, "listed twice"),
    ("err_quant_missing", None, "has no line"),
])
def test_refusals_through_the_command_line(golden_dir, tmp_path, name, line, why):
    """The deviations (dev_*: the reference writes a .bin) and the reference's own failures: exit 1, ``Error: <file> line <n>: <why>``,
    no file."""
    out = str(tmp_path / "o.bin")
    r = _cli([os.path.join(golden_dir, "salmon_" + name), out])
    assert r.returncode == 1, r.stderr[-2000:]
    err = [l for l in r.stderr.splitlines() if "Error:" in l]
    assert err and why in err[0], r.stderr[-2000:]
    if line is not None:
        assert " line %d:" % line in err[0], err[0]
    assert not os.path.exists(out)
    _good()


def test_random_directories_against_the_checker(tmp_path):
    """240 seeded directories: 1 - 31 haplotypes, shuffled names, 1 - 5 000 ECs, short and long rows, zero counts, empty rows, \\r\\n."""
    for seed in range(240):
        rng = np.random.default_rng(1000 + seed)
        H = int(rng.choice([1, 2, 3, 8, 16, 31]))
        n_tx = int(rng.integers(1, 200))
        E = int(rng.choice([1, 2, 7, 63, 64, 65, 500, 4097, 5000]))
        names = chk.target_names(n_tx, ["h%d" % h for h in range(H)], rng)
        eff = rng.uniform(0, 5000, size=len(names))
        ptr, tid, counts = chk.random_ecs(rng, len(names), E, mean_k=float(rng.uniform(1.5, 12)), long_every=int(rng.choice([0, 50])),
                                          long_k=(min(50, len(names)), min(len(names), 3000)))
        crlf = bool(rng.random() < 0.2)
        section = chk.ec_section(ptr, tid, counts, crlf=crlf)
        if rng.random() < 0.2 and section:
            section = section[:-2 if crlf else -1]                   # (no final line end)
        lname, hname, col, hap = chk.number_names(names)
        got = ecb.salmon_ecs(section, E, col, hap, len(lname), len(hname))
        exp = chk.expected(names, eff, ptr, tid, counts)
        _same(got, (exp[3], exp[4], exp[5], exp[7], exp[8]))
        if seed % 40 == 0:                                           # (and the whole command on some)
            d = str(tmp_path / ("s%d" % seed))
            chk.write_salmon_dir(d, names, eff, section, E)
            out = str(tmp_path / ("s%d.bin" % seed))
            salmon_utils.convert(d, out, "S")
            m = bin_utils.ECMatrices(exp[0], exp[1], exp[2], ["S"], *exp[3:])
            assert _bytes(out) == bin_utils.ecsave2_bytes(m), seed


def test_config3_sized_input_against_the_checker(tmp_path):
    """80 000 transcripts x 8 haplotypes, 3.7 M ECs, ~40 M target ids: the whole command against the checker."""
    rng = np.random.default_rng(33)
    names = chk.target_names(80_000, list("ABCDEFGH"), rng)
    eff = rng.uniform(0, 5000, size=len(names))
    E = 3_700_000
    ptr, tid, counts = chk.random_ecs_fast(rng, len(names), E)
    assert len(tid) > 35_000_000
    d = str(tmp_path / "c3")
    chk.write_salmon_dir(d, names, eff, chk.ec_section(ptr, tid, counts), E)
    out = str(tmp_path / "c3.bin")
    salmon_utils.convert(d, out, "c3")
    got = bin_utils.ecload(out)
    hname, lname, lengths, ip, ix, da, np_, nx, nd = chk.expected(names, eff, ptr, tid, counts)
    assert got.hname == hname and got.lname == lname and got.sname == ["c3"]
    assert np.array_equal(got.lengths.astype(np.int64), lengths)
    _same((got.indptrA, got.indicesA, got.dataA, got.indptrN, got.indicesN, got.dataN), (ip, ix, da, np_, nx, nd))


def _refuse(section, E, T=10, line=None, reason=None):
    col, hap = np.arange(T) // 2, np.arange(T) % 2
    with pytest.raises(ecb.SalmonFormatError) as e:
        ecb.salmon_ecs(section, E, col, hap, (T + 1) // 2, 2)
    assert (e.value.line, e.value.reason) == (line, reason), e.value.args
    if line is not None:
        with pytest.raises(chk.Refusal) as c:                        # (the checker agrees)
            chk.parse_section(section, E, T)
        assert (c.value.line, c.value.reason) == (line, reason)
    _good()


GOOD = b"2\t0\t1\t5\n1\t3\t7\n0\t2\n"


@pytest.mark.parametrize("bad,reason", [
    (b"2\t4\tx\t5\n", chk.R_BYTE), (b"2\t4\t5 \t5\n", chk.R_BYTE), (b"2\t4\r\t5\t5\n", chk.R_BYTE), (b"1\t4\t-5\n", chk.R_BYTE),
    (b"\t1\t4\t5\n", chk.R_EMPTY), (b"1\t4\t\t5\n", chk.R_EMPTY), (b"1\t4\t5\t\n", chk.R_EMPTY), (b"\n", chk.R_EMPTY), (b"\r\n", chk.R_EMPTY),
    (b"1\t4\t2147483648\n", chk.R_BIG), (b"1\t2147483648\t5\n", chk.R_BIG), (b"1\t4\t" + b"9" * 40 + b"\n", chk.R_BIG),
    (b"5\n", chk.R_FEW), (b"3\t1\t2\t5\n", chk.R_K), (b"0\t1\t5\n", chk.R_K), (b"1\t10\t5\n", chk.R_TARGET),
    (b"3\t1\t2\t1\t5\n", chk.R_REPEAT), (b"2\t9\t9\t5\n", chk.R_REPEAT),
])
def test_every_device_refusal_names_its_line(bad, reason):
    for before in (0, 2, 700):                                       # (the bad line in the first tile, and thousands of bytes in)
        text = GOOD * before + bad + GOOD
        _refuse(text, 3 * before + 4, line=3 * before, reason=reason)


def test_lowest_line_wins_whatever_the_reason():
    # a repeat (found after the sort) on line 1 and a bad byte on line 3: line 1; the reverse: line 1 again
    _refuse(b"1\t0\t5\n2\t3\t3\t1\n1\t0\t5\n1\tx\t5\n", 4, line=1, reason=chk.R_REPEAT)
    _refuse(b"1\t0\t5\n1\tx\t5\n1\t0\t5\n2\t3\t3\t1\n", 4, line=1, reason=chk.R_BYTE)
    _refuse(b"1\t0\t5\n2\t3\t3\t1\n", 9, line=1, reason=chk.R_REPEAT)          # (before the line count)
    _refuse(b"1\t0\t5\n1\t3\t1\n", 1, line=1, reason=chk.R_COUNT)
    _refuse(b"1\t0\t5\n1\t3\t1\n", 3, line=2, reason=chk.R_COUNT)
    _refuse(b"1\t0\t5\r", 1, line=0, reason=chk.R_BYTE)                          # (a \r at the end, not before a line end)


def test_long_fields_and_line_ends_at_every_offset():
    """Fields that run across thread (16 B) and workgroup (4 KB) boundaries: leading zeros, the last line without a line end."""
    col, hap = np.arange(10) // 2, np.arange(10) % 2
    for pad in (1, 15, 16, 17, 4095, 4096, 4097, 9000):
        text = b"1\t" + b"0" * pad + b"3\t" + b"0" * (pad // 2) + b"42\n2\t9\t8\t1"
        got = ecb.salmon_ecs(text, 2, col, hap, 5, 2)
        _same(got, ([0, 1, 2], [1, 4], [2, 3], [0, 1], [42, 1]))


def test_limits_and_arguments():
    col, hap = np.arange(4) // 2, np.arange(4) % 2
    with pytest.raises(ecb.EcbError) as e:                           # (a target map beyond n_loci)
        ecb.salmon_ecs(b"1\t0\t5\n", 1, col + 7, hap, 2, 2)
    assert e.value.code == ecb.ECB_ERR_CONTRACT
    with pytest.raises(ecb.EcbError) as e:
        ecb.salmon_ecs(b"1\t0\t5\n", 1, col, hap, 2, 32)
    assert e.value.code == -1
    _same(ecb.salmon_ecs(b"", 0, col, hap, 2, 2), ([0], [], [], [], []))
    _same(ecb.salmon_ecs(b"0\t0\n0\t3\n", 2, col, hap, 2, 2), ([0, 0, 0], [], [], [1], [3]))
    _good()


def test_device_entry_equals_host_entry(golden_dir):
    import torch
    d = os.path.join(golden_dir, "salmon_h8")
    data = _bytes(os.path.join(d, "aux_info", "eq_classes.txt"))
    h = salmon_utils.parse_header(data)
    lname, hname, col, hap = salmon_utils.number_targets(h.names)
    sec = data[h.ec_offset:]
    host = ecb.salmon_ecs(sec, h.n_ecs, col, hap, len(lname), len(hname))
    dev = ecb.salmon_ecs(torch.frombuffer(bytearray(sec), dtype=torch.uint8).cuda(), h.n_ecs, col, hap, len(lname), len(hname))
    assert all(t.is_cuda for t in dev)
    _same(dev, host)
    with pytest.raises(ecb.SalmonFormatError) as e:
        ecb.salmon_ecs(torch.frombuffer(bytearray(sec + b"0\t3\n"), dtype=torch.uint8).cuda(), h.n_ecs, col, hap, len(lname), len(hname))
    assert e.value.line == h.n_ecs and e.value.reason == chk.R_COUNT
