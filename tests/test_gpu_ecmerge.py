"""ecmerge on the GPU (``ecb_combine`` / ``ecb_combine_device``): g2 split by reads and converted part by part merges into the
reference's bytes through the command line; every golden alone comes back unchanged; target lists that differ are remapped; random
inputs, the apply-genotypes outputs and config-3-sized inputs against the checker or their construction; every contract violation
refused without harming the next call."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from alntools_amd import bamio, bin_utils, ecb, methods, synth

import ec_merge_checker as chk
import gt_checker

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDENS = ["g1_edge.bin", "g2_c1.bin", "g4_multi_min0.bin", "g4_multi_min20.bin", "g4_multi_min60.bin",
           "g4b_multi_min0.bin", "g4b_multi_min40.bin", "g4b_multi_min160.bin"]


def _bytes(p):
    with open(p, "rb") as f:
        return f.read()


def _same(got, exp):
    for g, e in zip(got, exp):
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert np.array_equal(np.asarray(g, dtype=np.int64), np.asarray(e, dtype=np.int64))


def _combine(ms):
    """ecb.combine over ECMatrices, planned as the command plans them -> ECMatrices."""
    plan = bin_utils.plan_merge(ms)
    parts = [dict(indptrA=m.indptrA, indicesA=m.indicesA, dataA=m.dataA, indptrN=m.indptrN, indicesN=m.indicesN, dataN=m.dataN,
                  n_loci=m.num_loci, target_map=tm, sample_map=sm) for m, tm, sm in zip(ms, plan.target_maps, plan.sample_maps)]
    return bin_utils.ECMatrices(plan.hname, plan.lname, plan.lengths, plan.sname,
                                *ecb.combine(parts, len(plan.lname), len(plan.hname), len(plan.sname)))


def test_g2_split_by_reads_merges_into_the_whole_through_the_command_line(golden_dir, tmp_path):
    g = json.load(open(os.path.join(golden_dir, "g2_c1.json")))
    spec = synth.SynthSpec(**g["spec"])
    env = dict(os.environ)
    env.pop("ALNTOOLS_TORCH", None)
    env.pop("ALNTOOLS_GPUS", None)
    for cuts in ([0, 5000, 10000], [0, 1, 3333, 6666, 9999, 10000]):
        bins = []
        for k, (r0, r1) in enumerate(zip(cuts[:-1], cuts[1:])):
            bam, b = str(tmp_path / ("p%d.bam" % k)), str(tmp_path / ("p%d_%d.bin" % (len(cuts), k)))
            bamio.write_bam(bam, spec.references(), synth.raw_records(spec, r0, r1), level=1)
            r = subprocess.run([sys.executable, "-m", "alntools_amd.cli", "bam2ec", bam, b, "-s", g["sample"]], cwd=ROOT, env=env,
                               capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
            bins.append(b)
        out = str(tmp_path / "merged.bin")
        args = sum((["-i", b] for b in bins), []) + ["-o", out, "-v"]
        r = subprocess.run([sys.executable, "-X", "importtime", "-m", "alntools_amd.cli", "ecmerge"] + args, cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        imported = [l.split("|")[-1].strip() for l in r.stderr.splitlines() if l.startswith("import time:")]
        assert "alntools_amd.ecb" in imported
        assert not any(m == "torch" or m.startswith("torch.") for m in imported)
        assert _bytes(out) == _bytes(os.path.join(golden_dir, "g2_c1.bin")), cuts


def test_every_golden_alone_comes_back_unchanged(golden_dir, tmp_path):
    for name in GOLDENS:
        out = str(tmp_path / name)
        methods.ecmerge([os.path.join(golden_dir, name)], out)
        assert _bytes(out) == _bytes(os.path.join(golden_dir, name)), name


@pytest.mark.parametrize("name", ["gt_c1.out.bin", "gt_c1_homA.out.bin", "gt_ms.out.bin", "gt_h8.out.bin"])
def test_apply_genotypes_outputs_alone_are_compacted_as_the_checker_does(golden_dir, tmp_path, name):
    p, out = os.path.join(golden_dir, name), str(tmp_path / "o.bin")
    methods.ecmerge([p], out)
    exp = chk.merge_bytes([bin_utils.ecload(p)])
    assert _bytes(out) == exp
    if name == "gt_c1.out.bin":
        assert bin_utils.ecload(out).num_reads < bin_utils.ecload(p).num_reads


def test_a_shuffled_target_list_is_remapped(golden_dir):
    rng = np.random.default_rng(11)
    a = bin_utils.ecload(os.path.join(golden_dir, "g4_multi_min0.bin"))
    b = bin_utils.ecload(os.path.join(golden_dir, "g4_multi_min20.bin"))
    whole = _combine([a, b])
    shuffled = _combine([a, chk.permute_targets(b, rng)])
    assert bin_utils.ecsave2_bytes(shuffled) == bin_utils.ecsave2_bytes(whole)
    assert bin_utils.ecsave2_bytes(whole) == chk.merge_bytes([a, b])
    c = chk.permute_targets(a, rng)
    c.sname = [s + "_x" for s in c.sname]
    got = _combine([a, c])
    assert got.num_samples == 2 * a.num_samples
    assert bin_utils.ecsave2_bytes(got) == chk.merge_bytes([a, c])


def test_random_inputs_against_the_checker_and_the_device_entry():
    import torch
    rng = np.random.default_rng(5)
    hname = ["A", "B", "C", "D", "E"]
    names = ["t%05d" % i for i in range(3000)]
    ms = [chk.random_bin(rng, 2500, names[:2000], hname, ["s1", "s2"]),
          chk.random_bin(rng, 1800, names[1000:], hname, ["s2", "s3", "s4"]),
          chk.random_bin(rng, 40, names[500:2500], hname, ["s5"], long_share=0.5),
          chk.random_bin(rng, 3000, names[:2000], hname, ["s1"], max_row=2000, long_share=0.01)]
    for m in ms[1:]:                                    # (a name's lengths agree everywhere)
        m.lengths = np.array([ms[0].lengths[names.index(t)] if names.index(t) < 2000 else np.arange(5) + names.index(t) for t in m.lname])
    ms[0].lengths = np.asarray(ms[0].lengths)
    assert max(np.diff(m.indptrA).max() for m in ms) > 1024
    for sub in (ms[:1], ms[1:2], ms[:2], ms, [ms[3], ms[0]]):
        got = _combine(sub)
        assert bin_utils.ecsave2_bytes(got) == chk.merge_bytes(sub)
    plan = bin_utils.plan_merge(ms)
    parts = [dict(indptrA=m.indptrA, indicesA=m.indicesA, dataA=m.dataA, indptrN=m.indptrN, indicesN=m.indicesN, dataN=m.dataN,
                  n_loci=m.num_loci, target_map=tm, sample_map=sm) for m, tm, sm in zip(ms, plan.target_maps, plan.sample_maps)]
    host = ecb.combine(parts, len(plan.lname), len(plan.hname), len(plan.sname))
    dparts = [{k: (torch.from_numpy(np.asarray(v, dtype=np.int32)).cuda() if isinstance(v, np.ndarray) else v) for k, v in p.items()} for p in parts]
    dev = ecb.combine(dparts, len(plan.lname), len(plan.hname), len(plan.sname))
    assert all(t.is_cuda for t in dev)
    _same(dev, host)


def _scale_parts(seed=3):
    ip, ix, da, T, H = gt_checker.c3_csr(seed)
    E = len(ip) - 1
    rng = np.random.default_rng(seed + 10)
    count = rng.integers(1, 100, size=E)
    ranges = [(0, 1_200_000), (900_000, 2_500_000), (2_000_000, E), (0, E)]
    share = rng.dirichlet(np.ones(4), size=E)
    parts = []
    left = count.copy()
    for k, (a, b) in enumerate(ranges):
        inside = np.zeros(E, bool)
        inside[a:b] = True
        if k < 3:
            c = np.where(inside, np.floor(count * share[:, k]).astype(np.int64), 0)
        else:
            c = left
        left = left - c
        rows = np.arange(a, b)
        pip = (ip[a:b + 1] - ip[a]).astype(np.int32)
        cr = c[a:b]
        nz = np.flatnonzero(cr)
        parts.append(dict(indptrA=pip, indicesA=ix[ip[a]:ip[b]], dataA=da[ip[a]:ip[b]], indptrN=np.array([0, len(nz)], np.int32),
                          indicesN=nz.astype(np.int32), dataN=cr[nz].astype(np.int32), n_loci=T, target_map=None,
                          sample_map=np.zeros(1, np.int32)))
        del rows
    assert not left.any()
    return (ip, ix, da, T, H, count), parts


def _row_hashes(ip, ix, da):
    """An independent 64-bit set hash per row (numpy): equal keys, equal hashes."""
    x = (ix.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) ^ (da.astype(np.uint64) * np.uint64(0xC2B2AE3D27D4EB4F))
    x ^= x >> np.uint64(29)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(32)
    lens = np.diff(ip).astype(np.int64)
    s = np.zeros(len(lens), dtype=np.uint64)
    nzr = lens > 0
    s[nzr] = np.add.reduceat(x, ip[:-1][nzr].astype(np.int64))
    return s + lens.astype(np.uint64) * np.uint64(0x100000001B3)


def test_config3_sized_inputs_with_overlapping_rows_and_split_counts():
    (ip, ix, da, T, H, count), parts = _scale_parts()
    whole = dict(indptrA=ip, indicesA=ix, dataA=da, indptrN=np.array([0, len(count)], np.int32), indicesN=np.arange(len(count), dtype=np.int32),
                 dataN=count.astype(np.int32), n_loci=T, target_map=None, sample_map=np.zeros(1, np.int32))
    exp = ecb.combine([whole], T, H, 1)
    got = ecb.combine(parts, T, H, 1)
    _same(got, exp)
    # the whole file's ECs, independently: one per distinct row key, in first-appearance order, each a row of the input, counts summed
    h = _row_hashes(ip, ix, da)
    uniq, first, inv = np.unique(h, return_index=True, return_inverse=True)
    order = np.sort(first)
    oip, oix, oda, nip, nix, nda = exp
    assert len(oip) - 1 == len(order)
    assert np.array_equal(_row_hashes(oip, oix, oda), h[order])
    assert np.array_equal(np.diff(oip), np.diff(ip)[order])
    rank = np.empty(len(uniq), np.int64)
    rank[np.argsort(first)] = np.arange(len(uniq))
    sums = np.bincount(rank[inv], weights=count, minlength=len(uniq)).astype(np.int64)
    assert np.array_equal(nix, np.flatnonzero(sums)) and np.array_equal(nda, sums[sums != 0])


def test_contract_violations_are_refused_and_the_next_call_works():
    rng = np.random.default_rng(9)
    hname = ["A", "B", "C"]
    names = ["t%d" % i for i in range(300)]
    a = chk.random_bin(rng, 500, names, hname, ["s"], max_row=200, long_share=0.05, empty_share=0.0)
    b = chk.random_bin(rng, 400, names, hname, ["s", "u"], max_row=200, long_share=0.05, empty_share=0.0)
    b.lengths = a.lengths
    good = chk.merge_bytes([a, b])
    plan = bin_utils.plan_merge([a, b])

    def parts(ma=a, tm=None, sm=None, **kw):
        p = [dict(indptrA=m.indptrA, indicesA=m.indicesA, dataA=m.dataA, indptrN=m.indptrN, indicesN=m.indicesN, dataN=m.dataN,
                  n_loci=m.num_loci, target_map=None, sample_map=s) for m, s in zip((ma, b), plan.sample_maps)]
        p[0].update(kw)
        if tm is not None:
            p[0]["target_map"] = tm
        if sm is not None:
            p[0]["sample_map"] = sm
        return p
    long_row = int(np.argmax(np.diff(a.indptrA)))
    s0 = int(a.indptrA[long_row])
    bad = []
    x = a.indicesA.copy(); x[5] = 300; bad.append(("column >= T", parts(indicesA=x), -5))
    x = a.indicesA.copy(); x[7] = -1; bad.append(("negative column", parts(indicesA=x), -5))
    d = a.dataA.copy(); d[9] = 8; bad.append(("bit >= H", parts(dataA=d), -5))
    d = a.dataA.copy(); d[11] = 0; bad.append(("stored 0", parts(dataA=d), -5))
    x = a.indicesA.copy(); x[s0 + 1], x[s0 + 2] = x[s0 + 2], x[s0 + 1]; bad.append(("unsorted column", parts(indicesA=x), -5))
    x = a.indicesA.copy(); x[s0 + 2] = x[s0 + 1]; bad.append(("duplicate column", parts(indicesA=x), -5))
    p_ = a.indptrA.copy(); p_[10], p_[11] = p_[11], p_[10]; bad.append(("falling indptr", parts(indptrA=p_), -5))
    p_ = a.indptrA.copy(); p_[-1] -= 1; bad.append(("indptr[E] != nnz", parts(indptrA=p_), -5))
    p_ = a.indptrA.copy(); p_[0] = 1; bad.append(("indptr[0] != 0", parts(indptrA=p_), -5))
    n = a.indicesN.copy(); n[3] = a.num_reads; bad.append(("EC index >= E", parts(indicesN=n), -5))
    n = a.dataN.copy(); n[4] = -2; bad.append(("negative count", parts(dataN=n), -5))
    p_ = a.indptrN.copy(); p_[-1] += 1; bad.append(("N pointers", parts(indptrN=p_), -5))
    tm = np.arange(300); tm[1] = 0; bad.append(("map not one-to-one", parts(tm=tm), -5))
    tm = np.arange(300); tm[4] = 300; bad.append(("map beyond T", parts(tm=tm), -5))
    bad.append(("sample map beyond S", parts(sm=np.array([7])), -5))
    n = a.dataN.copy(); n[:] = 2 ** 31 - 1; bad.append(("count sum beyond int32", [parts(dataN=n)[0], parts(dataN=n)[0]], -8))
    for what, p, code in bad:
        with pytest.raises(ecb.EcbError) as e:
            ecb.combine(p, len(plan.lname), len(plan.hname), len(plan.sname))
        assert e.value.code == code, what
        got = ecb.combine(parts(), len(plan.lname), len(plan.hname), len(plan.sname))   # the device is unharmed
        assert bin_utils.ecsave2_bytes(bin_utils.ECMatrices(plan.hname, plan.lname, plan.lengths, plan.sname, *got)) == good, what
