"""What every command does with a failure, without a GPU (the device calls replaced by stand-ins that hand the input back): the three
ways the ``Error: ...`` line and the exception go together -- a KeyError shown by its argument and raised again (``ecbundle``,
``ecselect``, ``count_alignments``; ``test_ecquant*`` pin the two ecquant commands), any exception shown by ``str()`` and raised again
(``ecmerge``, ``salmon2ec``), shown and swallowed as the reference does (``ecdump``; ``test_apply_genotypes`` pins the other) -- and
that a ``.bin`` whose write fails half-way is removed."""
import builtins
import os

import numpy as np
import pytest

from alntools_amd import bin_utils, ecb, salmon_utils

EC, GRP = "g4b_multi_min0.bin", "gt_ms.grp.txt"


def _same(ipa, ixa, daa, ipn, ixn, dan, *a, **k):
    return ipa, ixa, daa, ipn, ixn, dan


@pytest.fixture
def devices(monkeypatch):
    monkeypatch.setattr(ecb, "bundle", _same)
    monkeypatch.setattr(ecb, "select", lambda *a, **k: (_same(*a), np.ones(len(a[3]) - 1, dtype=bool)))
    monkeypatch.setattr(ecb, "combine", lambda parts, *a, **k: _same(*[parts[0][n] for n in ("indptrA", "indicesA", "dataA", "indptrN", "indicesN", "dataN")]))
    monkeypatch.setattr(salmon_utils, "parse_salmon_ec", lambda *a, **k: (["t0", "t1"], ["A"], np.array([[5], [7]]), ([0, 1, 2], [0, 1], [1, 1]),
                                                                          ([0, 2], [0, 1], [3, 4])))


def _commands(golden_dir, out):
    ec = os.path.join(golden_dir, EC)
    return {"ecbundle": lambda: bin_utils.ecbundle(ec, os.path.join(golden_dir, GRP), out),
            "ecselect": lambda: bin_utils.ecselect(ec, out),
            "ecmerge": lambda: bin_utils.ecmerge([ec, ec], out),
            "salmon2ec": lambda: salmon_utils.convert("nowhere", out)}


@pytest.mark.parametrize("name", ["ecbundle", "ecselect", "ecmerge", "salmon2ec"])
def test_a_bin_whose_write_fails_half_way_is_removed_and_the_failure_raised_again(golden_dir, tmp_path, monkeypatch, caplog, devices, name):
    out = str(tmp_path / "o.bin")
    real = builtins.open

    class HalfWritten(object):
        def __init__(self, fh):
            self.fh = fh

        def __enter__(self):
            return self

        def __exit__(self, *a):
            self.fh.close()

        def write(self, b):
            self.fh.write(b[:7])
            raise OSError("the disk is full")

    monkeypatch.setattr(builtins, "open", lambda p, *a, **k: HalfWritten(real(p, *a, **k)) if p == out else real(p, *a, **k))
    with caplog.at_level("INFO", logger="alntools.utils"):
        with pytest.raises(OSError, match="the disk is full"):
            _commands(golden_dir, out)[name]()
    monkeypatch.undo()
    assert not os.path.exists(out)
    assert "Error: the disk is full" in caplog.text and "created in" not in caplog.text and "Saving completed" not in caplog.text


@pytest.mark.parametrize("name", ["ecbundle", "ecselect", "ecmerge", "salmon2ec"])
def test_the_same_commands_write_the_file_and_say_so_when_nothing_fails(golden_dir, tmp_path, caplog, devices, name):
    out = str(tmp_path / "o.bin")
    with caplog.at_level("INFO", logger="alntools.utils"):
        _commands(golden_dir, out)[name]()
    assert bin_utils.ecload(out).num_haplotypes >= 1
    assert "Error" not in caplog.text and out + " created in " + ("total time: " if name != "salmon2ec" else "") in caplog.text


def test_a_key_error_is_shown_by_its_argument_and_raised_again(golden_dir, tmp_path, caplog, devices):
    ec, out = os.path.join(golden_dir, EC), str(tmp_path / "o")
    grp = str(tmp_path / "g.txt")
    with open(grp, "w") as fh:
        fh.write("G1\tTX_NOPE\n")
    for run, shown in ((lambda: bin_utils.ecbundle(ec, grp, out), "Error: TX_NOPE"),
                       (lambda: bin_utils.ecselect(ec, out, samples=["nobody"]), "Error: sample nobody is not in the EC file"),
                       (lambda: bin_utils.count_alignments(ec, out, sample="nobody"), "Error: sample nobody is not in " + ec)):
        caplog.clear()
        with caplog.at_level("ERROR", logger="alntools.utils"):
            with pytest.raises(KeyError):
                run()
        assert [r.getMessage() for r in caplog.records] == [shown] and not os.path.exists(out)


def test_ecmerge_and_salmon2ec_show_any_failure_as_str_does_and_raise_it_again(golden_dir, tmp_path, monkeypatch, caplog, devices):
    def refuse(*a, **k):
        raise KeyError("what str() puts in quotes")
    monkeypatch.setattr(ecb, "combine", refuse)
    monkeypatch.setattr(salmon_utils, "parse_salmon_ec", refuse)
    out = str(tmp_path / "o.bin")
    for name in ("ecmerge", "salmon2ec"):
        caplog.clear()
        with caplog.at_level("ERROR", logger="alntools.utils"):
            with pytest.raises(KeyError):
                _commands(golden_dir, out)[name]()
        assert [r.getMessage() for r in caplog.records] == ["Error: 'what str() puts in quotes'"] and not os.path.exists(out)


def test_ecdump_shows_a_failure_and_returns_as_the_reference_does(tmp_path, caplog):
    with caplog.at_level("ERROR", logger="alntools.utils"):
        assert bin_utils.ecdump(str(tmp_path / "missing.bin")) is None
    assert len(caplog.records) == 1 and caplog.records[0].getMessage().startswith("Error: [Errno 2]")
