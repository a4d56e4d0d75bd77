#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""Generate the salmon2ec fixtures (``salmon_*``) in this directory by RUNNING THE REFERENCE.

Build-container only, like ``make_golden_gt.py``: writes hand-made salmon directories (``salmon_<case>/aux_info/eq_classes.txt``,
``quant.sf``, and for ``-t`` a ``targets.tsv``) from seeded arrays, imports the unmodified reference package from ``/root/reference``
with the stand-ins of ``_standins/`` ahead of it, runs its ``salmon_utils.convert`` on each, and records data only:

  salmon_cases.json        every case: its directory, sample, target file, the .bin the reference wrote (or null) and the exception
                           it raised (type and message)
  salmon_<case>.bin        what the reference wrote

    python tests/golden/make_golden_salmon.py
"""
from __future__ import print_function

import json
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.join(HERE, "_standins"))

import numpy as np  # noqa: E402

import salmon_checker as chk  # noqa: E402  (the writer)
from alntools import salmon_utils  # noqa: E402  (the reference)


def case_dir(name):
    d = os.path.join(HERE, "salmon_" + name)
    if os.path.exists(d):
        shutil.rmtree(d)
    return d


def write(name, names, eff, section, n_ecs, quant_names=None, targets=None, header_extra=b""):
    d = case_dir(name)
    chk.write_salmon_dir(d, names, eff, section, n_ecs, header_extra=header_extra)
    if quant_names is not None:                                   # a quant.sf of other names (the refusals)
        with open(os.path.join(d, "quant.sf"), "w") as fh:
            fh.write("Name\tLength\tEffectiveLength\tTPM\tNumReads\n")
            for n, e in quant_names:
                fh.write("%s\t100\t%s\t1.0\t1.0\n" % (n, e))
    if targets is not None:
        with open(os.path.join(d, "targets.tsv"), "w") as fh:
            fh.write("".join(t + "\textra\n" for t in targets))
    return d


def random_case(name, seed, n_tx, haps, n_ecs, shuffle=True, crlf=False, **kw):
    rng = np.random.default_rng(seed)
    names = chk.target_names(n_tx, haps, rng if shuffle else None)
    eff = np.round(rng.uniform(0.0, 3000.0, size=len(names)), 3)
    ptr, tid, counts = chk.random_ecs(rng, len(names), n_ecs, **kw)
    return names, eff, chk.ec_section(ptr, tid, counts, crlf=crlf), n_ecs


def small(lines, n_ecs=None, names=("T1_A", "T1_B", "T2_B", "T2_A", "T3_A", "T0_B")):
    names = list(names)
    eff = [80.7, 80.2, 150.9, 151.0, 0.5, 20.0][:len(names)] + [10.0] * max(0, len(names) - 6)
    return names, eff, b"".join(lines), len(lines) if n_ecs is None else n_ecs


def main():
    cases = []

    def add(name, d, sample="NA", targets=None, note=""):
        out = os.path.join(HERE, "salmon_%s.bin" % name)
        if os.path.exists(out):
            os.remove(out)
        tmp = tempfile.mkdtemp()
        got, err = os.path.join(tmp, "out.bin"), None
        try:
            salmon_utils.convert(d, got, sample, os.path.join(d, targets) if targets else None)
            shutil.copy(got, out)
        except Exception as e:                                      # noqa: BLE001  (what the reference raised, recorded)
            err = {"type": type(e).__name__, "message": str(e)}
        shutil.rmtree(tmp)
        cases.append({"name": name, "dir": os.path.basename(d), "sample": sample, "targets": targets,
                      "bin": os.path.basename(out) if err is None else None, "error": err, "note": note})
        print(name, "->", "error %s" % err if err else os.path.basename(out))

    # conversions the reference completes
    add("diploid", write("diploid", *random_case("diploid", 1, 40, ["A", "B"], 300)), sample="S1")
    add("h8", write("h8", *random_case("h8", 2, 60, list("HCAFBGED"), 400)), note="8 haplotypes, names not in sorted order")
    names, eff, sec, E = random_case("targets", 3, 20, ["A", "B"], 100)
    add("targets", write("targets", names, eff, sec, E, targets=["TX000003", "NEW1", "TX000000", "NEW2", "NEW1"]), targets="targets.tsv",
        note="-t with new and already-present names")
    add("zero", write("zero", *small([b"2\t0\t1\t10\n", b"0\t7\n", b"1\t4\t0\n", b"3\t3\t2\t5\t0\n", b"0\t0\n", b"2\t1\t0\t3\n"])),
        note="zero counts and lines without targets")
    rng = np.random.default_rng(5)
    names = chk.target_names(1500, ["A", "B"], rng)
    eff = rng.uniform(1, 2000, size=len(names))
    ptr = np.array([0, 2, 3002, 3005])
    tid = np.concatenate([[0, 1], rng.choice(len(names), size=3000, replace=False), [5, 6, 7]])
    add("long", write("long", names, eff, chk.ec_section(ptr, tid, [4, 9, 1]), 3), note="one EC of 3 000 targets")
    add("frac", write("frac", ["T1_A", "T1_B", "T2_A", "T2_B", "T3_B"], [80.7, 0.5, 0.999, 1.0, 1234.56789],
                      b"2\t0\t1\t3\n1\t4\t2\n3\t2\t3\t1\t1\n", 3), note="fractional and sub-1 effective lengths")
    add("crlf", write("crlf", *random_case("crlf", 7, 10, ["A", "B"], 50, crlf=True)), note="\\r\\n line ends in the EC section")
    # what the reference accepts and this project refuses: recorded so that the deviation is pinned
    add("dev_k", write("dev_k", *small([b"2\t0\t1\t10\n", b"5\t4\t3\n"])), note="k differs from the number of target ids")
    add("dev_repeat", write("dev_repeat", *small([b"2\t0\t1\t10\n", b"2\t4\t4\t3\n"])), note="a target id twice in one line")
    add("dev_fewer", write("dev_fewer", *small([b"2\t0\t1\t10\n", b"1\t4\t3\n"], n_ecs=4)), note="fewer EC lines than E")
    add("dev_quant_dup", write("dev_quant_dup", *small([b"1\t0\t5\n"], names=("T1_A", "T1_B")),
                               quant_names=[("T1_A", "10"), ("T1_B", "20"), ("T1_B", "30")]),
        note="a quant.sf name twice, its target in no EC (when one uses it the reference raises)")
    # what the reference raises on
    add("err_no_underscore", write("err_no_underscore", *small([b"1\t0\t5\n"], names=("T1_A", "T1B"))))
    add("err_two_underscores", write("err_two_underscores", *small([b"1\t0\t5\n"], names=("T1_A", "T1_B_C"))))
    add("err_header_dup", write("err_header_dup", *small([b"1\t0\t5\n"], names=("T1_A", "T1_B", "T1_A"))))
    add("err_quant_missing", write("err_quant_missing", *small([b"1\t0\t5\n"], names=("T1_A", "T1_B")), quant_names=[("T1_A", "10")]))
    add("err_quant_extra", write("err_quant_extra", *small([b"1\t0\t5\n"], names=("T1_A", "T1_B")),
                                 quant_names=[("T1_A", "10"), ("T1_B", "20"), ("T9_A", "30")]))
    add("err_more_lines", write("err_more_lines", *small([b"1\t0\t5\n", b"1\t1\t5\n", b"1\t2\t5\n"], n_ecs=2)))
    add("err_target_id", write("err_target_id", *small([b"1\t0\t5\n", b"2\t1\t6\t5\n"])))
    add("err_letter", write("err_letter", *small([b"1\t0\t5\n", b"2\t1\tx\t5\n"])))
    add("err_empty_line", write("err_empty_line", *small([b"1\t0\t5\n", b"\n", b"1\t2\t5\n"])))
    add("err_empty_field", write("err_empty_field", *small([b"1\t0\t5\n", b"2\t1\t\t2\t5\n"])))
    with open(os.path.join(HERE, "salmon_cases.json"), "w") as fh:
        json.dump(cases, fh, indent=1)


if __name__ == "__main__":
    main()
