"""apply-genotypes on the GPU (``ecb_apply_mask`` / ``ecb_apply_mask_device``): the reference's bytes through the Python function and the
command line, the device entry against the host entry, random and config-3-sized CSRs against the numpy checker, and every contract
violation refused without harming the next call."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from alntools_amd import bamio, bin_utils, ecb, methods

import gt_checker

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _bytes(p):
    with open(p, "rb") as f:
        return f.read()


def _ok_cases(golden_dir):
    return [c for c in json.load(open(os.path.join(golden_dir, "gt_cases.json")))["cases"] if c["out"]]


def _same(got, exp):
    for g, e in zip(got, exp):
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert np.array_equal(np.asarray(g, dtype=np.int64), np.asarray(e, dtype=np.int64))


def test_goldens_through_apply_genotypes(golden_dir, tmp_path):
    for c in _ok_cases(golden_dir):
        out = str(tmp_path / (c["name"] + ".bin"))
        methods.apply_genotypes(*[os.path.join(golden_dir, c[k]) for k in ("ec", "gt", "grp")], out)
        assert _bytes(out) == _bytes(os.path.join(golden_dir, c["out"])), c["name"]


def test_goldens_through_the_command_line_import_no_pytorch(golden_dir, tmp_path):
    env = dict(os.environ)
    env.pop("ALNTOOLS_TORCH", None)
    env.pop("ALNTOOLS_GPUS", None)
    for c in _ok_cases(golden_dir):
        out = str(tmp_path / (c["name"] + ".bin"))
        args = [os.path.join(golden_dir, c[k]) for k in ("ec", "gt", "grp")] + [out, "-v"]
        r = subprocess.run([sys.executable, "-X", "importtime", "-m", "alntools_amd.cli", "apply-genotypes"] + args, cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        imported = [l.split("|")[-1].strip() for l in r.stderr.splitlines() if l.startswith("import time:")]
        assert "alntools_amd.ecb" in imported
        assert not any(m == "torch" or m.startswith("torch.") for m in imported)
        assert "Error:" not in r.stderr, r.stderr[-2000:]
        assert _bytes(out) == _bytes(os.path.join(golden_dir, c["out"])), c["name"]


def test_device_entry_equals_host_entry(golden_dir):
    import torch
    c = {c["name"]: c for c in _ok_cases(golden_dir)}["h8"]
    m = bin_utils.ecload(os.path.join(golden_dir, c["ec"]))
    mask = np.array(c["mask"], dtype=np.uint32)
    host = ecb.apply_mask(m.indptrA, m.indicesA, m.dataA, mask, m.num_haplotypes)
    dev = ecb.apply_mask(*[torch.from_numpy(a.astype(np.int32)).cuda() for a in (m.indptrA, m.indicesA, m.dataA, mask)], m.num_haplotypes)
    assert all(t.is_cuda for t in dev)
    _same(dev, host)
    _same(host, gt_checker.mask_csr(m.indptrA, m.indicesA, m.dataA, mask))


@pytest.mark.parametrize("n_haps", [1, 2, 8, 31])
def test_random_csrs_against_the_checker(n_haps):
    rng = np.random.default_rng(100 + n_haps)
    for n_ecs, n_loci in ((1, 1), (1, 900), (7, 3), (4097, 1000), (16_385, 2_000), (70_001, 5_000)):
        ip, ix, da = gt_checker.random_csr(rng, n_ecs, n_loci, n_haps)
        full = (1 << n_haps) - 1
        for mask in (rng.integers(0, full + 1, size=n_loci, dtype=np.int64).astype(np.uint32),
                     np.zeros(n_loci, dtype=np.uint32), np.full(n_loci, full, dtype=np.uint32)):
            got = ecb.apply_mask(ip, ix, da, mask, n_haps)
            _same(got, gt_checker.mask_csr(ip, ix, da, mask))
            assert len(got[0]) == n_ecs + 1


def test_empty_rows_only_and_no_non_zeros():
    ip = np.zeros(6, dtype=np.int32)
    got = ecb.apply_mask(ip, np.zeros(0, np.int32), np.zeros(0, np.int32), np.ones(4, np.uint32), 2)
    _same(got, (ip, [], []))


def test_config3_sized_csr_against_the_checker():
    ip, ix, da, T, H = gt_checker.c3_csr()
    rng = np.random.default_rng(7)
    mask = rng.integers(0, 1 << H, size=T, dtype=np.int64).astype(np.uint32)
    _same(ecb.apply_mask(ip, ix, da, mask, H), gt_checker.mask_csr(ip, ix, da, mask))


def test_contract_violations_are_refused_and_the_next_call_works():
    rng = np.random.default_rng(5)
    ip, ix, da = gt_checker.random_csr(rng, 3000, 500, 4)
    mask = np.full(500, 0b0101, dtype=np.uint32)
    good = gt_checker.mask_csr(ip, ix, da, mask)
    long_row = int(np.argmax(np.diff(ip)))
    a = int(ip[long_row])
    bad = []
    x = ix.copy(); x[5] = 500; bad.append(("locus >= T", ip, x, da, mask))
    x = ix.copy(); x[7] = -1; bad.append(("negative locus", ip, x, da, mask))
    d = da.copy(); d[9] = 16; bad.append(("bit >= H", ip, ix, d, mask))
    m = mask.copy(); m[3] = 1 << 4; bad.append(("mask bit >= H", ip, ix, da, m))
    x = ix.copy(); x[a + 1], x[a + 2] = x[a + 2], x[a + 1]; bad.append(("unsorted column", ip, x, da, mask))
    x = ix.copy(); x[a + 2] = x[a + 1]; bad.append(("duplicate column", ip, x, da, mask))
    p = ip.copy(); p[10], p[11] = p[11], p[10]; bad.append(("falling indptr", p, ix, da, mask))
    p = ip.copy(); p[-1] -= 1; bad.append(("indptr[E] != nnz", p, ix, da, mask))
    p = ip.copy(); p[0] = 1; bad.append(("indptr[0] != 0", p, ix, da, mask))
    p = ip.copy(); p[20] = len(ix) + 5; bad.append(("indptr beyond nnz", p, ix, da, mask))
    for what, p, x, d, m in bad:
        with pytest.raises(ecb.EcbError) as e:
            ecb.apply_mask(p, x, d, m, 4)
        assert e.value.code == -5, what                        # ECB_ERR_CONTRACT
        _same(ecb.apply_mask(ip, ix, da, mask, 4), good)       # the device is unharmed


def test_bam2ec_apply_genotypes_ec2emase_emase2ec_round_trip(golden_dir, tmp_path):
    """g1 BAM -> .bin -> genotypes applied -> EMASE .h5 -> .bin again: the masked .bin comes back.  Its haplotypes are '', A, B: no
    genotype character names '', so that haplotype always goes."""
    from alntools_amd import emase_h5
    try:
        emase_h5._backend()
    except RuntimeError:
        pytest.skip("no HDF5 library on this box")
    g = json.load(open(os.path.join(golden_dir, "g1_edge.json")))
    bam = str(tmp_path / g["sample"])
    bamio.write_bam(bam, [tuple(r) for r in g["references"]], [tuple(r) for r in g["records"]])
    b1, b2, h5, b3 = (str(tmp_path / n) for n in ("a.bin", "b.bin", "b.h5", "c.bin"))
    methods.bam2ec(bam, b1)
    m = bin_utils.ecload(b1)
    assert m.hname == ["", "A", "B"]
    grp, gt = str(tmp_path / "grp.txt"), str(tmp_path / "gt.txt")
    open(grp, "w").write("G1\t{}\t{}\nG2\t{}\n".format(m.lname[0], m.lname[1], m.lname[2]))
    open(gt, "w").write("# genotypes\nG1\tAB\nG2\tBB\n")
    methods.apply_genotypes(b1, gt, grp, b2)
    mk = np.zeros(m.num_loci, dtype=np.uint32)
    mk[[0, 1]], mk[2] = 0b110, 0b100
    exp = gt_checker.mask_csr(m.indptrA, m.indicesA, m.dataA, mk)
    got = bin_utils.ecload(b2)
    _same((got.indptrA, got.indicesA, got.dataA), exp)
    assert not (got.dataA & 1).any()
    methods.ec2emase(b2, h5)
    methods.emase2ec(h5, b3)
    assert _bytes(b3) == _bytes(b2)
