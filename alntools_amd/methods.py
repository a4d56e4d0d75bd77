# -*- coding: utf-8 -*-
"""Same driver functions as the reference's ``alntools/methods.py:32-53, 205-210``, ``apply_genotypes``, ``ecmerge``, ``ecbundle``, ``ecselect``, ``ecdownsample``, ``salmon2ec``, ``bus2ec``, ``buscorrect``, ``count_alignments``, ``ecquant``, ``ecboot``, ``ecclusters``, ``ecquant_cells`` and ``ecdump`` for the hot path."""
from __future__ import annotations

from . import bam_utils, bin_utils


def bam2ec(bam_filename, ec_filename, chunks=0, directory=None, number_processes=-1, range_filename=None,
           sample=None, target_filename=None, best_strata=None):
    return bam_utils.convert(bam_filename, ec_filename, None, num_chunks=chunks, number_processes=number_processes,
                             temp_dir=directory, range_filename=range_filename, sample=sample,
                             target_filename=target_filename, best_strata=best_strata)


def bam2emase(bam_filename, emase_filename, chunks=0, directory=None, number_processes=-1, range_filename=None,
              target_filename=None, best_strata=None):
    return bam_utils.convert(bam_filename, None, emase_filename, num_chunks=chunks, number_processes=number_processes,
                             temp_dir=directory, range_filename=range_filename, target_filename=target_filename, best_strata=best_strata)


def bam2both(bam_filename, ec_filename, emase_filename, chunks=0, directory=None, number_processes=-1,
             range_filename=None, sample=None, target_filename=None):
    return bam_utils.convert(bam_filename, ec_filename, emase_filename, num_chunks=chunks,
                             number_processes=number_processes, temp_dir=directory, range_filename=range_filename,
                             sample=sample, target_filename=target_filename)


def bam2ec_multisample(bam_filename, ec_filename, chunks=0, minimum_count=-1, directory=None, number_processes=-1,
                       range_filename=None, target_filename=None, best_strata=None, collapse_umis=False):
    from . import bam_utils_multisample
    return bam_utils_multisample.convert(bam_filename, ec_filename, None, chunks, minimum_count, number_processes,
                                         directory, range_filename, target_filename, best_strata=best_strata, collapse_umis=collapse_umis)


def bam2emase_multisample(bam_filename, emase_filename, chunks=0, minimum_count=-1, directory=None,
                          number_processes=-1, range_filename=None, target_filename=None, best_strata=None, collapse_umis=False):
    from . import bam_utils_multisample
    return bam_utils_multisample.convert(bam_filename, None, emase_filename, chunks, minimum_count, number_processes,
                                         directory, range_filename, target_filename, best_strata=best_strata, collapse_umis=collapse_umis)


def ec2emase(ec_file, emase_file):
    bin_utils.ec2emase(ec_file, emase_file)


def emase2ec(emase_file, ec_file):
    bin_utils.emase2ec(emase_file, ec_file)


def apply_genotypes(ec_file, gt_file, grp_file, out_file):
    bin_utils.apply_genotypes(ec_file, gt_file, grp_file, out_file)


def ecmerge(input_files, out_file):
    bin_utils.ecmerge(input_files, out_file)


def ecbundle(ec_file, grp_file, out_file):
    bin_utils.ecbundle(ec_file, grp_file, out_file)


def ecdownsample(ec_file, out_file, reads=None, fraction=None, equalize=False, seed=0, samples=None, samples_file=None, mincount=None, stats_file=None):
    bin_utils.ecdownsample(ec_file, out_file, reads=reads, fraction=fraction, equalize=equalize, seed=seed, samples=samples,
                           samples_file=samples_file, mincount=mincount, stats_file=stats_file)


def ecselect(ec_file, out_file, row_class=None, samples=None, samples_file=None, mincount=None):
    bin_utils.ecselect(ec_file, out_file, row_class=row_class, samples=samples, samples_file=samples_file, mincount=mincount)


def count_alignments(ec_file, out_file, sample=None):
    bin_utils.count_alignments(ec_file, out_file, sample=sample)


def ecquant(ec_file, out_file, sample=None, use_lengths=False, max_iters=1000, tol=1e-6, model=4, groups=None, posterior_file=None):
    named = {} if posterior_file is None else {"posterior_file": posterior_file}
    bin_utils.ecquant(ec_file, out_file, sample=sample, use_lengths=use_lengths, max_iters=max_iters, tol=tol, model=model, groups=groups, **named)


def ecboot(ec_file, out_file, n_boot=None, seed=0, sample=None, use_lengths=False, max_iters=1000, tol=1e-6, model=4, groups=None, replicates_file=None):
    bin_utils.ecboot(ec_file, out_file, n_boot=n_boot, seed=seed, sample=sample, use_lengths=use_lengths, max_iters=max_iters, tol=tol, model=model,
                     groups=groups, replicates_file=replicates_file)


def ecclusters(ec_file, out_file, sample=None, min_count=1, stats_file=None, multi_only=False):
    bin_utils.ecclusters(ec_file, out_file, sample=sample, min_count=min_count, stats_file=stats_file, multi_only=multi_only)


def ecquant_cells(ec_file, out_file, samples=None, samples_file=None, use_lengths=False, max_iters=1000, tol=1e-6, report=None, model=4, groups=None):
    bin_utils.ecquant_cells(ec_file, out_file, samples=samples, samples_file=samples_file, use_lengths=use_lengths, max_iters=max_iters, tol=tol,
                            report=report, model=model, groups=groups)


def ecdump(ec_file):
    bin_utils.ecdump(ec_file)


def salmon2ec(salmon_dir, ec_filename, sample=None, target_filename=None):
    from . import salmon_utils
    salmon_utils.convert(salmon_dir, ec_filename, sample='NA' if sample is None else sample, target_filename=target_filename)


def bus2ec(bus_dir, ec_filename, no_umi=False, mincount=1000, names_file=None, lengths_file=None, haplotype=None, target_filename=None, stats_file=None,
           whitelist_file=None):
    from . import bus_utils
    bus_utils.convert(bus_dir, ec_filename, no_umi=no_umi, mincount=mincount, names_file=names_file, lengths_file=lengths_file, haplotype=haplotype,
                      target_filename=target_filename, stats_file=stats_file, whitelist_file=whitelist_file)


def buscorrect(bus_file, out_file, whitelist_file, stats_file=None):
    from . import bus_utils
    bus_utils.correct_file(bus_file, out_file, whitelist_file, stats_file=stats_file)
