"""ecboot without a GPU: the checker (``tests/boot_checker.py``) against Random123's known answers, its replicates' sanity statistic, the draw
file (``alntools_amd/csrc/boot_draw.h``) compiled as plain C++ against the checker's Python integers, the ABI's header against the module's
symbols, the kernel constants the GPU tests place their shapes on, the table writer and the command with the bindings stood in."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from alntools_amd import bin_utils, ecb, ecb_boot

import boot_checker as bc

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "alntools_amd", "csrc")
C1 = os.path.join(GOLDEN, "g2_c1.bin")
MS = os.path.join(GOLDEN, "g4b_multi_min0.bin")
TPB, BS_DRAWS = 256, 8                      # what the GPU tests import ...
BS_WG_DRAWS = TPB * BS_DRAWS                # ... and the workgroup's draws
_loaded = {}


@pytest.fixture(autouse=True)
def _logger_level_as_it_was():
    import logging
    log = logging.getLogger("alntools.utils")
    level = log.level
    yield
    log.setLevel(level)


def load(path):
    if path not in _loaded:
        _loaded[path] = bin_utils.ecload(path)
    return _loaded[path]


def weights_of(path, sample=None):
    m = load(path)
    return bc.weights(m.num_reads, m.indptrN, m.indicesN, m.dataN, sample)


# ---- 1. Random123's known answers ------------------------------------------------------------------------------------------------------------
KAT = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("counter,key,want", KAT, ids=["zeros", "ones", "pi"])
def test_the_checkers_philox_gives_random123s_known_answers(counter, key, want):
    assert " ".join("%08x" % int(v) for v in bc.philox(counter, key)) == want


# ---- 2. the sanity statistic -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,W,B", [(C1, 9593, 64), (MS, 20355, 32)], ids=["g2_c1", "g4b_pooled"])
@pytest.mark.parametrize("seed", [0, 1])
def test_replicates_sum_to_w_skip_weightless_rows_and_scatter_as_a_multinomial(path, W, B, seed):
    w = weights_of(path)
    assert int(w.sum()) == W
    ptr, ec, cnt, dense = bc.resample(w, seed, 0, B)
    assert (dense.sum(axis=1) == W).all() and not dense[:, w == 0].any()
    assert ptr[-1] == len(ec) == len(cnt) and (cnt > 0).all()
    z = bc.z_statistic(dense, w)
    print("%s seed %d: z = %.3f" % (os.path.basename(path), seed, z))
    assert abs(z) < 4


# ---- 3. the draw file as plain C++ -----------------------------------------------------------------------------------------------------------
MAIN = r"""
#include <cinttypes>
#include <cstdio>
#include "boot_draw.h"
int main() {
    unsigned long long seed, b, i, W;
    while (std::scanf("%llu %llu %llu %llu", &seed, &b, &i, &W) == 4)
        std::printf("%" PRIu32 "\n", bs_draw_x((uint64_t)seed, (uint32_t)b, (uint32_t)i, (uint32_t)W));
    return 0;
}
"""


def test_the_draw_file_compiled_for_the_host_gives_the_checkers_x(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    (tmp_path / "main.cc").write_text(MAIN)
    exe = str(tmp_path / "draw")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", exe, str(tmp_path / "main.cc")])
    seeds = [0, 1, 1 << 32, 1 << 63, (1 << 63) + 12345, (1 << 32) + 12345, 12345, (1 << 64) - 1]
    cases = [(s, b, i, W) for s in seeds for b in (0, 7, (1 << 32) - 1) for W in (1, 2, 3, 9593, (1 << 31) - 1)
             for i in sorted(i for i in {0, 1, 2, 3, W - 2, W - 1} if 0 <= i < W)]
    out = subprocess.run([exe], input="".join("%d %d %d %d\n" % c for c in cases), capture_output=True, text=True, check=True).stdout.split()
    want = [bc.draw_x(*c) for c in cases]
    assert [int(v) for v in out] == want
    assert all(0 <= x < c[3] for x, c in zip(want, cases))
    by = dict(zip(cases, want))
    W = (1 << 31) - 1
    # seeds that differ in bit 32 or in bit 63 alone draw differently: both key words are used
    assert by[(12345, 0, 0, W)] != by[((1 << 32) + 12345, 0, 0, W)] and by[(12345, 0, 0, W)] != by[((1 << 63) + 12345, 0, 0, W)]
    assert by[(0, 0, 0, W)] != by[(0, (1 << 32) - 1, 0, W)] and by[(0, 0, 0, W)] != by[(0, 0, 1, W)]
    # the vectorised draws the other tests use are these
    assert list(bc.xs(1 << 63, 7, 9593)[[0, 1, 2, 3, 9591, 9592]]) == [by[(1 << 63, 7, i, 9593)] for i in (0, 1, 2, 3, 9591, 9592)]


# ---- 4. the header, the constants, the table, the command ------------------------------------------------------------------------------------
def test_the_header_declares_exactly_the_modules_symbols():
    text = open(os.path.join(ROOT, "include", "ecb_quant_boot.h")).read()
    declared = re.findall(r"^int (ecb_\w+)\(", text, re.M)
    assert sorted(declared) == sorted(ecb_boot.BOOT_SYMBOLS) and len(set(declared)) == 4
    assert '#include "ecb_quant_boot.h"' in open(os.path.join(ROOT, "include", "ecb_quant.h")).read()
    bound = [n for name, _, _, twin, _ in ecb_boot.BOOT_SIGNATURES for n in ((name + "_device", name) if twin else (name,))]
    assert sorted(bound) == sorted(ecb_boot.BOOT_SYMBOLS)
    assert not set(ecb_boot.BOOT_SYMBOLS) & set(ecb.SYMBOLS) and not {s[0] for s in ecb.SIGNATURES} & {s[0] for s in ecb_boot.BOOT_SIGNATURES}
    for name, argtypes, _, _, _ in ecb_boot.BOOT_SIGNATURES:          # as many parameters as the prototype has
        proto = re.search(r"^int %s\((.*?)\);" % name, text, re.M | re.S).group(1)
        assert len(proto.split(",")) == len(argtypes), name
    from alntools_amd import build
    assert any(p.endswith("ecb_quant_boot.h") for p in build.inputs()) and any(p.endswith("boot_draw.h") for p in build.inputs())
    assert any(p.endswith("boot.inc") for p in build.inputs())


def test_constants_the_ecboot_tests_straddle():
    src = open(os.path.join(CSRC, "boot.inc")).read()
    assert re.findall(r"constexpr\s+u32\s+BS_DRAWS\s*=\s*([^;,]+);", src) == [str(BS_DRAWS)], "move test_gpu_ecboot.py's W around the workgroup's draws"
    assert re.findall(r"constexpr\s+u32\s+BS_WG_DRAWS\s*=\s*([^;,]+);", src) == ["TPB * BS_DRAWS"]
    assert re.findall(r"constexpr\s+int\s+TPB\s*=\s*(\d+);", open(os.path.join(CSRC, "ecb.hip")).read()) == [str(TPB)]
    assert "atomicAdd(reinterpret_cast<double" not in src and "unsafeAtomicAdd" not in src and "atomicAdd(double" not in src      # no float atomics
    assert len(re.findall(r"qc_run\(", src)) == 2 and "k_qc_estep" not in src and "k_q_estep" not in src                      # a composition: no EM of its own


def test_the_table_has_the_estimate_with_mean_and_sd_beside_it():
    theta = np.array([[1.5, 0.0], [2.25, 1e-300]])
    mean, sd = theta + 0.5, theta * 0.1
    text = bin_utils.boot_table(["t0", "t1"], ["A", "B"], theta, mean, sd, [4.0, 0.5], [0.25, 0.0])
    lines = text.split("\n")
    assert lines[0] == "locus\tA\tA_mean\tA_sd\tB\tB_mean\tB_sd\ttotal\ttotal_mean\ttotal_sd" and lines[3] == "" and len(lines) == 4
    assert lines[1].split("\t") == ["t0", "1.5", "2.0", str(1.5 * 0.1), "2.25", "2.75", str(2.25 * 0.1), "3.75", "4.0", "0.25"]
    row = lines[2].split("\t")
    assert row[0] == "t1" and [float(v) for v in row[1:]] == [0.0, 0.5, 0.0, 1e-300, 1e-300 + 0.5, 1e-300 * 0.1, 1e-300, 0.5, 0.0]
    # the point-estimate columns are ecquant's table
    q = [ln.split("\t") for ln in bin_utils.quant_table(["t0", "t1"], ["A", "B"], theta).split("\n")[1:3]]
    assert [[r[1], r[4], r[7]] for r in (lines[1].split("\t"), row)] == [r[1:] for r in q]


def _stand_ins(monkeypatch, calls):
    def quantify(*a, **kw):
        calls.append(("quantify", kw))
        return np.full((a[4], a[3]), 2.0), {"n_iter": 3, "delta": 0.0, "explained": 7, "converged": True}

    def quantify_model(*a, **kw):
        calls.append(("quantify_model", kw))
        return np.full((a[4], a[3]), 3.0), {"n_iter": 3, "delta": 0.0, "explained": 7, "converged": True}

    def quantify_bootstrap(*a, **kw):
        calls.append(("bootstrap", kw))
        H, T, B = a[4], a[3], kw["n_reps"]
        info = {"n_iter": np.full(B, 2), "delta": np.zeros(B), "explained": np.zeros(B, dtype=np.int64), "converged": np.ones(B, dtype=bool)}
        out = (np.full((H, T), 1.0), np.full((H, T), 0.5), np.full(T, 2.0), np.full(T, 0.75), info)
        return out + ((np.arange(B * H * T, dtype=np.float64).reshape(B, H, T),) if kw["return_reps"] else ())
    monkeypatch.setattr(ecb, "quantify", quantify)
    monkeypatch.setattr(ecb, "quantify_model", quantify_model)
    monkeypatch.setattr(ecb_boot, "quantify_bootstrap", quantify_bootstrap)


def test_the_command_with_the_bindings_stood_in(tmp_path, monkeypatch):
    from click.testing import CliRunner
    from alntools_amd import cli
    calls = []
    _stand_ins(monkeypatch, calls)
    out, npy = str(tmp_path / "boot.tsv"), str(tmp_path / "reps.npy")
    r = CliRunner().invoke(cli.cli, ["ecboot", C1, out, "-b", "3", "--seed", str((1 << 63) + 5), "-i", "20", "-t", "1e-4", "--replicates", npy])
    assert r.exit_code == 0, r.output
    m = load(C1)
    assert [c[0] for c in calls] == ["quantify", "bootstrap"]
    kw = calls[1][1]
    assert (kw["n_reps"], kw["seed"], kw["sample"], kw["max_iters"], kw["tol"], kw["model"], kw["gene"], kw["scale"]) == (3, (1 << 63) + 5, None, 20, 1e-4, 4, None, None)
    assert (calls[0][1]["max_iters"], calls[0][1]["tol"], calls[0][1]["sample"]) == (20, 1e-4, None)
    lines = open(out).read().split("\n")
    assert lines[0].split("\t") == ["locus"] + [c for h in m.hname for c in (h, h + "_mean", h + "_sd")] + ["total", "total_mean", "total_sd"]
    assert len(lines) == m.num_loci + 2 and lines[1].split("\t") == [m.lname[0]] + ["2.0", "1.0", "0.5"] * m.num_haplotypes + [str(2.0 * m.num_haplotypes), "2.0", "0.75"]
    assert np.array_equal(np.load(npy), np.arange(3 * m.num_haplotypes * m.num_loci, dtype=np.float64).reshape(3, m.num_haplotypes, m.num_loci))
    # a model with its group file goes to quantify_model and on to the bootstrap, -l as a scale
    del calls[:]
    monkeypatch.setattr(ecb, "count_alignments", lambda *a, **kw: (np.ones((a[4], a[3]), dtype=np.int64),) * 2 + (None,))
    grp = os.path.join(GOLDEN, "quant_model_c1.grp.txt")
    r = CliRunner().invoke(cli.cli, ["ecboot", C1, out, "-b", "2", "-M", "2", "-g", grp, "-l"])
    assert r.exit_code == 0, r.output
    assert [c[0] for c in calls] == ["quantify_model", "bootstrap"]
    kw = calls[1][1]
    assert kw["model"] == 2 and kw["seed"] == 0 and kw["gene"].shape == (m.num_loci,) and kw["n_genes"] == calls[0][1]["n_genes"] > 0
    assert kw["scale"].shape == (m.num_haplotypes, m.num_loci) and kw["return_reps"] is False
    assert "ecboot" in cli.__doc__ and "alntools ecboot sample.bin boot.tsv -b" in open(os.path.join(ROOT, "README.md")).read()


@pytest.mark.parametrize("argv,text", [
    (["-b", "0"], None), ([], None), (["-b", "2", "-M", "2"], "needs a group file"), (["-b", "2", "-s", "nobody"], "sample nobody is not in"),
], ids=["b0", "no-b", "model-without-groups", "unknown-sample"])
def test_a_refused_command_exits_with_1_or_a_usage_error_and_writes_no_file(tmp_path, monkeypatch, argv, text, caplog):
    from click.testing import CliRunner
    from alntools_amd import cli
    _stand_ins(monkeypatch, [])
    out, npy = str(tmp_path / "boot.tsv"), str(tmp_path / "reps.npy")
    r = CliRunner().invoke(cli.cli, ["ecboot", C1, out, "--replicates", npy] + argv)
    assert r.exit_code == (1 if text else 2), r.output
    assert not os.path.exists(out) and not os.path.exists(npy)
    if text:
        assert any(text in rec.getMessage() and rec.getMessage().startswith("Error: ") for rec in caplog.records)


def test_a_failure_behind_the_first_file_removes_it(tmp_path, monkeypatch):
    _stand_ins(monkeypatch, [])
    out, npy = str(tmp_path / "no-such-dir" / "boot.tsv"), str(tmp_path / "reps.npy")
    with pytest.raises(OSError):
        bin_utils.ecboot(C1, out, n_boot=2, replicates_file=npy)
    assert not os.path.exists(npy)
    with pytest.raises(ValueError):
        bin_utils.ecboot(C1, str(tmp_path / "b.tsv"), n_boot=0)
    with pytest.raises(ValueError):
        bin_utils.ecboot(C1, str(tmp_path / "b.tsv"), n_boot=1, seed=1 << 64)
    assert os.listdir(str(tmp_path)) == []
