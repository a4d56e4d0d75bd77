"""Barcode correction on the CPU: the checker (``tests/bus_correct_checker.py``) held to a hand-written dozen of records whose expected
statuses are spelled out here, ``bus_utils.read_whitelist`` with every refusal and its line, the header and the bindings, ``--stats``
with and without the four new lines, and the command line's two faces of it."""
import gzip
import os
import re

import numpy as np
import pytest

from alntools_amd import bus_utils

import bus_checker as bc
import bus_correct_checker as cc

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

# ---- the hand-written dozen ---------------------------------------------------------------------------------------------------------------
WHITE = ["AAAA", "AAAC", "CCCC", "GGGG", "TTTT"]
HAND = [   # barcode, status, barcode afterwards
    ("AAAA", 0, "AAAA"),     # on the list -- that AAAC, one base away, is on it too does not matter
    ("AAAG", 3, None),       # AAAA and AAAC: two candidates at one position
    ("CCCA", 1, "CCCC"),     # the last base
    ("ACGT", 2, None),       # nothing within one base
    ("GGGT", 1, "GGGG"),
    ("TTTT", 0, "TTTT"),
    ("TATT", 1, "TTTT"),     # an inner base
    ("CACA", 2, None),       # two bases from CCCC
    ("AAAT", 3, None),
    ("AACC", 1, "AAAC"),     # one base from AAAC, two from CCCC and from AAAA
    ("CCCC", 0, "CCCC"),
    ("GGGG", 0, "GGGG"),
]


def _hand():
    n = len(HAND)
    return bc.records(np.array([bc.encode(h[0]) for h in HAND], dtype=np.uint64), np.arange(n, dtype=np.uint64) + np.uint64(100), np.arange(n) % 5,
                      np.arange(n) + 1, flags=7)


def test_the_checker_on_the_hand_written_dozen():
    rec = _hand()
    status, kept, sizes = cc.correct(rec, 4, [bc.encode(w) for w in WHITE])
    assert status.tolist() == [0, 3, 1, 2, 1, 0, 1, 2, 3, 1, 0, 0] == [h[1] for h in HAND] and set(status.tolist()) == {0, 1, 2, 3}
    assert sizes == (4, 4, 2, 2)
    want = [(bc.encode(h[2]), 100 + i, i % 5, i + 1) for i, h in enumerate(HAND) if h[2] is not None]
    assert [tuple(x) for x in zip(*bc.fields(kept))] == want and len(kept) == 8
    # the other 24 bytes are the input's
    assert np.array_equal(kept[:, 8:], rec[[i for i, h in enumerate(HAND) if h[2] is not None], 8:])
    assert len(cc.neighbours("ACGT")) == 12 == len(set(cc.neighbours("ACGT"))) and all(cc.distance(s, "ACGT") == 1 for s in cc.neighbours("ACGT"))
    assert cc.outcome(bc.encode("T" * 32), 32, {bc.encode("G" + "T" * 31)}) == (1, bc.encode("G" + "T" * 31))
    assert cc.outcome(bc.encode("T" * 32), 32, {bc.encode("T" * 31 + "A"), bc.encode("A" + "T" * 31)})[0] == 3


# ---- read_whitelist -------------------------------------------------------------------------------------------------------------------------
def _wl(tmp_path, data, name="wl.txt"):
    p = str(tmp_path / name)
    with (gzip.open if name.endswith(".gz") else open)(p, "wb") as fh:
        fh.write(data)
    return p


def test_read_whitelist_plain_gzipped_without_a_final_newline_and_with_crlf(tmp_path):
    want = np.array(sorted(bc.encode(s) for s in ("GATT", "ACGT", "TTTT", "AAAA")), dtype=np.uint64)
    for data, name in ((b"GATT\nACGT\nTTTT\nAAAA\n", "a.txt"), (b"GATT\nACGT\nTTTT\nAAAA", "b.txt"), (b"GATT\r\nACGT\r\nTTTT\r\nAAAA\r\n", "c.txt"),
                       (b"GATT\r\nACGT\r\nTTTT\r\nAAAA", "d.txt"), (b"GATT\nACGT\nTTTT\nAAAA\n", "e.txt.gz")):
        got = bus_utils.read_whitelist(_wl(tmp_path, data, name), 4)
        assert got.dtype == np.uint64 and np.array_equal(got, want), name
    top = "T" + "A" * 30 + "C"
    assert bus_utils.read_whitelist(_wl(tmp_path, (top + "\n" + "A" * 32 + "\n").encode()), 32).tolist() == [0, (3 << 62) | 1]
    rng = np.random.default_rng(1)
    seqs = sorted(set("".join(rng.choice(list("ACGT"), size=16)) for _ in range(3000)))
    rng.shuffle(seqs)
    got = bus_utils.read_whitelist(_wl(tmp_path, "\n".join(seqs).encode(), "many.txt.gz"), 16)
    assert got.tolist() == sorted(bus_utils.encode(s) for s in seqs)


@pytest.mark.parametrize("data,bclen,what", [
    (b"ACGT\nACGN\n", 4, "line 2: barcode 'ACGN' has a letter outside ACGT"),
    (b"ACGT\nacgt\n", 4, "line 2: barcode 'acgt' has a letter outside ACGT"),
    (b"ACGT\nACG\nAC\n", 4, "line 2: barcode 'ACG' has 3 bases; the BUS file's have 4"),
    (b"ACGT\nACGTA\n", 4, "line 2: barcode 'ACGTA' has 5 bases; the BUS file's have 4"),
    (b"ACGT\n\nAAAA\n", 4, "line 2: barcode '' has 0 bases; the BUS file's have 4"),
    (b"ACGT\nAAAA\nTTTT\nAAAA\nACGT\n", 4, "line 4: barcode 'AAAA' is listed twice (first on line 2)"),
    (b"ACGT\r\nACGT\r\n", 4, "line 2: barcode 'ACGT' is listed twice (first on line 1)"),
    (b"", 4, "no barcodes"),
])
def test_read_whitelist_refuses_with_the_file_and_the_line(tmp_path, data, bclen, what):
    for name in ("wl.txt", "wl.txt.gz"):
        p = _wl(tmp_path, data, name)
        with pytest.raises(ValueError) as e:
            bus_utils.read_whitelist(p, bclen)
        assert str(e.value).startswith(p) and what in str(e.value), str(e.value)


# ---- the header and the bindings --------------------------------------------------------------------------------------------------------------
def test_the_header_declares_exactly_the_modules_symbols():
    from alntools_amd import build, ecb, ecb_bus, ecb_bus_correct
    text = open(os.path.join(ROOT, "include", "ecb_bus_correct.h")).read()
    declared = re.findall(r"^int (ecb_\w+)\(", text, re.M)
    assert sorted(declared) == sorted(ecb_bus_correct.BUS_CORRECT_SYMBOLS) == ["ecb_bus_correct", "ecb_bus_correct_device"] and len(declared) == 2
    main = open(os.path.join(ROOT, "include", "ecb.h")).read()
    assert len(re.findall(r'^#\s*include "ecb_bus_correct\.h"', main, re.M)) == 1 and "ECB_ABI_VERSION 4" in main and "ABI 4, additive" in text
    assert main.index('include "ecb_bus.h"') < main.index('include "ecb_bus_correct.h"')
    bound = [n for name, _, _, twin, _ in ecb_bus_correct.BUS_CORRECT_SIGNATURES for n in ((name + "_device", name) if twin else (name,))]
    assert sorted(bound) == sorted(ecb_bus_correct.BUS_CORRECT_SYMBOLS) and len(ecb_bus_correct.BUS_CORRECT_SIGNATURES) == 1
    assert not set(bound) & (set(ecb.SYMBOLS) | set(ecb_bus.BUS_SYMBOLS))
    for name, argtypes, _, _, _ in ecb_bus_correct.BUS_CORRECT_SIGNATURES:          # as many parameters as the prototypes have
        for n in (name, name + "_device"):
            proto = re.search(r"^int %s\((.*?)\);" % n, text, re.M | re.S).group(1)
            assert len(proto.split(",")) == len(argtypes) == 10, n
    assert any(p.endswith("ecb_bus_correct.h") for p in build.inputs()) and any(p.endswith("bus_correct.inc") for p in build.inputs())
    hip = open(os.path.join(ROOT, "alntools_amd", "csrc", "ecb.hip")).read()
    assert len(re.findall(r'^#include "bus_correct\.inc"', hip, re.M)) == 1 and hip.index('#include "bus.inc"') < hip.index('#include "bus_correct.inc"')
    for k, name in enumerate(("EXACT", "CORRECTED", "NO_CANDIDATE", "AMBIGUOUS")):
        assert re.search(r"#define ECB_BUS_%s %du\b" % (name, k), text) and getattr(ecb_bus_correct, name) == k
    assert issubclass(ecb_bus_correct.WhitelistFormatError, ecb_bus.BusFormatError)


def test_the_stats_file_with_and_without_the_whitelists_lines():
    s = dict(records=12, molecules=7, molecules_in_several_ecs=3, molecules_discarded=1, new_ecs=1, cells=2, cells_kept=2)
    seven = "records\t12\nmolecules\t7\nmolecules_in_several_ecs\t3\nmolecules_discarded\t1\nnew_ecs\t1\ncells\t2\ncells_kept\t2\n"
    assert bus_utils.stats_text(s) == seven
    s.update(barcodes_exact=9, barcodes_corrected=1, barcodes_without_candidate=2, barcodes_ambiguous=0)
    assert bus_utils.stats_text(s) == seven + "barcodes_exact\t9\nbarcodes_corrected\t1\nbarcodes_without_candidate\t2\nbarcodes_ambiguous\t0\n"
    assert bus_utils.WHITELIST_STATS == ("barcodes_exact", "barcodes_corrected", "barcodes_without_candidate", "barcodes_ambiguous")


def test_the_command_line_has_the_option_and_the_command(tmp_path):
    from click.testing import CliRunner
    from alntools_amd import cli, methods
    assert "``buscorrect``" in cli.__doc__ and "``buscorrect``" in methods.__doc__ and {"bus2ec", "buscorrect"} <= set(cli.cli.commands)
    assert {"-w", "--whitelist"} <= {o for p in cli.cli.commands["bus2ec"].params for o in p.opts}
    assert {"-w", "--whitelist", "--stats", "-v"} <= {o for p in cli.cli.commands["buscorrect"].params for o in p.opts}
    run = CliRunner()
    r = run.invoke(cli.cli, ["bus2ec", "--help"])
    assert r.exit_code == 0 and "--whitelist" in r.output and "--names" in r.output
    r = run.invoke(cli.cli, ["buscorrect", "--help"])
    assert r.exit_code == 0 and "--whitelist" in r.output and "bus_file" in r.output and "out_file" in r.output
    src = str(tmp_path / "in.bus")
    open(src, "wb").close()
    r = run.invoke(cli.cli, ["buscorrect", src, str(tmp_path / "out.bus")])
    assert r.exit_code == 2 and "-w" in r.output and "issing option" in r.output and not os.path.exists(str(tmp_path / "out.bus"))
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "alntools buscorrect" in readme and "bus2ec" in readme and "--whitelist" in readme
