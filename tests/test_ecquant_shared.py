# -*- coding: utf-8 -*-
"""The five ecquant sources (``alntools_amd/csrc/quant*.inc``) share one validation front, one column view, one gene view and one driver
for the paths that are not per cell: each of them is written out once, in the file whose kernels it launches.  No GPU."""
from __future__ import annotations

import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "alntools_amd", "csrc")
FILES = ["quant.inc", "quant_cells.inc", "quant_cells_model.inc", "quant_model.inc", "quant_post.inc"]


def _body(src, head):
    """The text of the function whose definition starts with ``head``, up to the closing brace in column 0."""
    assert src.count(head) == 1, head
    return src.split(head)[1].split("\n}\n")[0]


def test_the_front_the_views_and_the_driver_each_stand_once_across_the_five_files():
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "quant*.inc"))) == FILES
    src = {f: open(os.path.join(CSRC, f)).read() for f in FILES}
    everything = "\n".join(src[f] for f in FILES)
    # the validation front: q_front in quant.inc, called by the driver, by the per-cell driver and by the posterior
    front = _body(src["quant.inc"], "int q_front(")
    for launch in (r"k_gm_check<true><<<", r"k_ca_weights<<<"):
        assert len(re.findall(launch, everything)) == 1 and len(re.findall(launch, front)) == 1
    assert len(re.findall(r"k_q_tab<<<", everything)) == 2 and len(re.findall(r"k_q_tab<<<", front)) == 2          # (scale, theta)
    assert len(re.findall(r"ca_refuse_input\(", everything)) == 1 and len(re.findall(r"2\^32-1 set haplotype bits", front)) == 1
    assert [f for f in FILES if re.search(r"\bq_front\(c, ", src[f])] == ["quant.inc", "quant_cells.inc", "quant_post.inc"]
    assert len(re.findall(r"\bq_front\(c, ", everything)) == 3
    # the column view: q_col_view in quant.inc
    assert len(re.findall(r"k_cv_keys<<<", everything)) == 1 and "k_cv_keys<<<" in _body(src["quant.inc"], "int q_col_view(")
    # the gene view: qm_gene_view in quant_model.inc, for the models (through qm_setup) and for the posterior
    assert len(re.findall(r"k_qm_rkeys<<<", everything)) == 1 and "k_qm_rkeys<<<" in _body(src["quant_model.inc"], "int qm_gene_view(")
    assert len(re.findall(r"k_qm_glist<<<", everything)) == 1
    assert [f for f in FILES if re.search(r"\bqm_gene_view\(c, ", src[f])] == ["quant_model.inc", "quant_post.inc"] and len(re.findall(r"\bqm_gene_view\(c, ", everything)) == 2
    # the chain of the models: qm_step in quant_model.inc, for the models' loop and, once, for the posterior
    step = _body(src["quant_model.inc"], "void qm_step(")
    for launch in (r"k_qm_gh<<<", r"k_qm_g<<<", r"k_qm_seg1<<<", r"k_qm_row<<<", r"k_qm_mstep<<<"):
        assert len(re.findall(launch, everything)) == 1 and len(re.findall(launch, step)) == 1
    assert len(re.findall(r"k_qm_gkeys<<<", everything)) == 2             # (the front; model 4's check of the genes alone, one helper for both families)
    assert len(re.findall(r"k_qm_gkeys<<<", _body(src["quant_model.inc"], "int qm_check_genes("))) == 1
    # the driver of the paths that are not per cell: q_run in quant.inc, with its loop of Q_BATCH steps between two looks; qc_run has the other
    run = _body(src["quant.inc"], "int q_run(")
    assert len(re.findall(r"for \(u32 queued = 0; !fin\.done;\)", everything)) == 1 and len(re.findall(r"for \(u32 queued = 0; !fin\.done;\)", run)) == 1
    assert len(re.findall(r"k < Q_BATCH && queued < max_iters", everything)) == 2
    assert len(re.findall(r"k < Q_BATCH && queued < max_iters", run)) == 1 and len(re.findall(r"k < Q_BATCH && queued < max_iters", src["quant_cells.inc"])) == 1
    assert len(re.findall(r"k_q_conv<<<", everything)) == 1 and len(re.findall(r"k_q_out<<<", everything)) == 1 and len(re.findall(r"k_q_arm<<<", everything)) == 1
