# -*- coding: utf-8 -*-
"""Command line with the reference's hot-path sub-commands and options (``alntools/cli.py:43-113``):
``bam2ec``, ``bam2emase``, ``ec2emase``, ``emase2ec``, ``apply-genotypes``, ``ecmerge``, ``ecbundle``, ``ecselect``, ``ecdownsample``, ``salmon2ec``, ``bus2ec`` (``-w``: the barcodes corrected against a whitelist first), ``buscorrect``, ``count-alignments``, ``ecquant`` (``-w``: the posterior of every alignment too), ``ecboot``, ``ecclusters``, ``ecquant-cells``, ``ecdump``.  ``python -m alntools_amd.cli bam2ec in.bam out.bin``."""
from __future__ import annotations

import glob
import os
import sys

import click

# The one-GPU commands move everything through libecb's host-pointer entry points: no tensors, so PyTorch is not imported and libecb
# runs on the system's HIP runtime (alntools_amd/ecb.py: load).  ALNTOOLS_GPUS=N (> 1) runs ranks over torch.distributed and wants it.
if int(os.environ.get("ALNTOOLS_GPUS", "1") or 1) <= 1:
    os.environ.setdefault("ALNTOOLS_TORCH", "0")

from . import methods, utils  # noqa: E402


@click.group()
def cli():
    """alntools hot path on MI355X (libecb)."""


def _common(f):
    for opt in (click.option('-v', '--verbose', count=True, help='enables verbose mode'),
                click.option('-t', '--targets', default=None, type=click.Path(exists=True, dir_okay=False), help='target file'),
                click.option('--rangefile', default=None, type=click.Path(dir_okay=False), help='range file'),
                click.option('-p', '--number-processes', '--processes', 'processes', default=-1,
                             help='number of processes (accepted for compatibility: the work runs on the GPU)'),
                click.option('--multisample', is_flag=True, help='BAM_FILE is a directory of per-sample BAM files'),
                click.option('-m', '--mincount', default=None, type=int, help='minimum reads per cell (multisample)'),
                click.option('--best-strata', 'best_strata', default=None, metavar='TAG',
                             help="keep only a read's best-scoring alignments: NM, XM, nM (lowest), AS, AS+YS (highest)"),
                click.option('--collapse-umis', 'collapse_umis', is_flag=True,
                             help="count molecules, not reads: reads of one cell with one UMI ('|||' field 6 of the read name) become one (multisample)"),
                click.option('-d', '--directory', default=None, type=click.Path(file_okay=False), help='accepted for compatibility; ignored'),
                click.option('-c', '--chunks', default=0, help='accepted for compatibility; ignored')):
        f = opt(f)
    return f


def _umi_option(collapse_umis, multisample, rangefile):
    """``--collapse-umis`` as the keyword the multisample drivers take (nothing without the option: the call is then today's); what the
    option does not run with is refused here, by name, before a file is opened or a process started."""
    if not collapse_umis:
        return {}
    from .bam_utils_multisample import umi_refusal
    why = umi_refusal(multisample, rangefile)
    if why:
        click.echo("Error: {}".format(why), err=True)
        sys.exit(1)
    return {"collapse_umis": True}


def _strata_option(tag):
    """``--best-strata TAG`` as the keyword the drivers take (nothing without the option: the call is then today's); an unknown TAG and
    ``ALNTOOLS_GPUS`` above 1 are refused here, by name, before a file is opened or a process started."""
    if tag is None:
        return {}
    from .ecb_strata import TAGS
    if tag not in TAGS:
        click.echo("Error: --best-strata {}: the tag is one of {}".format(tag, ", ".join(TAGS)), err=True)
        sys.exit(1)
    if int(os.environ.get("ALNTOOLS_GPUS", "1") or 1) > 1:
        click.echo("Error: --best-strata does not run with ALNTOOLS_GPUS above 1", err=True)
        sys.exit(1)
    return {"best_strata": tag}


class _strata_errors(object):
    """What ``--best-strata`` (a passing record without the tag) and ``--collapse-umis`` (a run beyond the record limit) refuse while
    they run: ``Error: ...``, exit status 1, no output file."""

    def __enter__(self):
        return self

    def __exit__(self, kind, e, tb):
        from .bam_utils import BestStrataError
        from .bam_utils_multisample import CollapseUmisError
        if kind is not None and issubclass(kind, (BestStrataError, CollapseUmisError)):
            click.echo("Error: {}".format(e), err=True)
            sys.exit(1)
        return False


@cli.command('bam2ec', short_help='convert a BAM file to EC')
@click.argument('bam_file', metavar='bam_file', type=click.Path(exists=True, resolve_path=True))
@click.argument('ec_file', metavar='ec_file', type=click.Path(resolve_path=True, dir_okay=False))
@click.option('-s', '--sample', default=None, help='sample identifier')
@_common
def bam2ec(bam_file, ec_file, chunks, directory, best_strata, collapse_umis, mincount, multisample, processes, rangefile, targets, verbose, sample):
    """Convert a BAM file (bam_file) to a binary file (ec_file)."""
    utils.configure_logging(verbose)
    named = _strata_option(best_strata)
    umis = _umi_option(collapse_umis, multisample, rangefile)
    if multisample:
        if sample:                                                   # cli.py:60-63
            print('-s, --sample should NOT be specified with --multisample')
            return
        with _strata_errors():
            methods.bam2ec_multisample(bam_file, ec_file, chunks, 1000 if mincount is None else mincount, directory,
                                       processes, rangefile, targets, **named, **umis)
    else:
        with _strata_errors():
            methods.bam2ec(bam_file, ec_file, chunks, directory, processes, rangefile, sample, targets, **named)


@cli.command('bam2emase', short_help='convert a BAM file to EMASE')
@click.argument('bam_file', metavar='bam_file', type=click.Path(exists=True, resolve_path=True))
@click.argument('emase_file', metavar='emase_file', type=click.Path(resolve_path=True, dir_okay=False))
@_common
def bam2emase(bam_file, emase_file, chunks, directory, best_strata, collapse_umis, mincount, multisample, processes, rangefile, targets, verbose):
    """Convert a BAM file (bam_file) to an EMASE file (emase_file)."""
    utils.configure_logging(verbose)
    named = _strata_option(best_strata)
    umis = _umi_option(collapse_umis, multisample, rangefile)
    with _strata_errors():
        if multisample:
            methods.bam2emase_multisample(bam_file, emase_file, chunks, 2000 if mincount is None else mincount, directory,
                                          processes, rangefile, targets, **named, **umis)
        else:
            methods.bam2emase(bam_file, emase_file, chunks, directory, processes, rangefile, targets, **named)


@cli.command('ec2emase', short_help='convert an EC file to EMASE')
@click.argument('ec_file', metavar='ec_file', type=click.Path(exists=True, resolve_path=True, dir_okay=False))
@click.argument('emase_file', metavar='emase_file', type=click.Path(resolve_path=True, dir_okay=False))
@click.option('-v', '--verbose', count=True, help='enables verbose mode')
def ec2emase(ec_file, emase_file, verbose):
    utils.configure_logging(verbose)
    methods.ec2emase(ec_file, emase_file)


@cli.command('emase2ec', short_help='convert an EMASE file to EC')
@click.argument('emase_file', metavar='emase_file', type=click.Path(exists=True, resolve_path=True, dir_okay=False))
@click.argument('ec_file', metavar='ec_file', type=click.Path(resolve_path=True, dir_okay=False))
@click.option('-v', '--verbose', count=True, help='enables verbose mode')
def emase2ec(emase_file, ec_file, verbose):
    utils.configure_logging(verbose)
    methods.emase2ec(emase_file, ec_file)


@cli.command('apply-genotypes', options_metavar='<options>', short_help='remove alignments inconsistent to the genotypes')
@click.argument('ec_file', metavar='ec_file', type=click.Path(exists=True, resolve_path=True, dir_okay=False))
@click.argument('gt_file', metavar='gt_file', type=click.Path(resolve_path=True, dir_okay=False))
@click.argument('grp_file', metavar='grp_file', type=click.Path(resolve_path=True, dir_okay=False))
@click.argument('out_file', metavar='out_file', type=click.Path(resolve_path=True, dir_okay=False))
@click.option('-v', '--verbose', count=True, help='enables verbose mode')
def apply_genotypes(ec_file, gt_file, grp_file, out_file, verbose):
    """
    Apply genotypes (gt_file) to an alignment profile in a binary EC format (ec_file)
    """
    utils.configure_logging(verbose)
    methods.apply_genotypes(ec_file, gt_file, grp_file, out_file)


@cli.command('ecmerge', options_metavar='<options>', short_help='merge multiple ec files')
@click.option('-i', '--input', 'inputs', metavar='input', type=click.Path(exists=True, resolve_path=True, dir_okay=False), multiple=True,
              help="input file, can specify multiple")
@click.option('-d', '--directory', metavar='directory', type=click.Path(exists=True, resolve_path=True, file_okay=False, dir_okay=True),
              help="input directory (its *.bin files, in name order, after the -i files)")
@click.option('-o', '--output', metavar='output', required=True, type=click.Path(resolve_path=True, dir_okay=False), help="output file")
@click.option('-v', '--verbose', count=True, help='the more times listed, the more output')
def ecmerge(inputs, directory, output, verbose):
    """
    Combine binary EC files
    """
    utils.configure_logging(verbose)
    input_files = list(inputs)
    if directory:
        bin_files = sorted(glob.glob(os.path.join(directory, "*.bin")))
        if len(bin_files) == 0:
            print('No bin files found in directory: {}'.format(directory))
            sys.exit(1)
        input_files.extend(bin_files)
    try:
        methods.ecmerge(input_files, output)
    except Exception:
        sys.exit(1)                                                  # (logged as "Error: ..." by bin_utils.ecmerge)


@cli.command('ecbundle', options_metavar='<options>', short_help='collapse the targets of an EC file into groups')
@click.argument('ec_file', metavar='ec_file', type=click.Path(exists=True, resolve_path=True, dir_okay=False))
@click.argument('grp_file', metavar='grp_file', type=click.Path(exists=True, resolve_path=True, dir_okay=False))
@click.argument('out_file', metavar='out_file', type=click.Path(resolve_path=True, dir_okay=False, writable=True))
@click.option('-v', '--verbose', count=True, help='enables verbose mode')
def ecbundle(ec_file, grp_file, out_file, verbose):
    """
    Collapse the targets of a binary EC file (ec_file) into the groups of grp_file (isoforms into genes) and write the result (out_file)
    """
    utils.configure_logging(verbose)
    try:
        methods.ecbundle(ec_file, grp_file, out_file)
    except Exception:
        sys.exit(1)                                                  # (logged as "Error: ..." by bin_utils.ecbundle)


@cli.command('ecselect', options_metavar='<options>', short_help='keep a class of reads and the samples that still count them')
@click.argument('ec_file', metavar='ec_file', type=click.Path(exists=True, resolve_path=True, dir_okay=False))
@click.argument('out_file', metavar='out_file', type=click.Path(resolve_path=True, dir_okay=False, writable=True))
@click.option('--unique', 'classes', flag_value='unique', multiple=True, help='keep the reads with one alignment to one haplotype')
@click.option('--locus-unique', 'classes', flag_value='locus-unique', multiple=True, help='keep the reads that align to one target')
@click.option('--multi', 'classes', flag_value='multi', multiple=True, help='keep the reads that align to two targets or more')
@click.option('-s', '--sample', 'samples', metavar='NAME', multiple=True, help="sample to keep, can specify multiple (default: all)")
@click.option('--samples', 'samples_file', metavar='FILE', type=click.Path(exists=True, resolve_path=True, dir_okay=False),
              help="file with the names of the samples to keep, one per line")
@click.option('-m', '--mincount', default=None, type=int, help='drop the samples that count fewer reads than this')
@click.option('-v', '--verbose', count=True, help='enables verbose mode')
def ecselect(ec_file, out_file, classes, samples, samples_file, mincount, verbose):
    """
    Pull a class of reads and the samples that still count enough of them out of a binary EC file (ec_file) and write the result (out_file)
    """
    if len(classes) > 1:
        raise click.UsageError('at most one of --unique, --locus-unique and --multi')
    utils.configure_logging(verbose)
    try:
        methods.ecselect(ec_file, out_file, classes[0] if classes else None, list(samples) or None, samples_file, mincount)
    except Exception:
        sys.exit(1)                                                  # (logged as "Error: ..." by bin_utils.ecselect)


@cli.command('ecdownsample', options_metavar='<options>', short_help='thin the samples of an EC file to a read depth')
@click.argument('ec_file', metavar='ec_file', type=click.Path(exists=True, resolve_path=True, dir_okay=False))
@click.argument('out_file', metavar='out_file', type=click.Path(resolve_path=True, dir_okay=False, writable=True))
@click.option('-n', '--reads', 'reads', metavar='N', default=None, type=int, help='keep N reads of every sample (a sample of fewer keeps all)')
@click.option('-f', '--fraction', 'fraction', metavar='P', default=None, type=float, help="keep floor(P x reads) of every sample's reads (0 < P <= 1)")
@click.option('--equalize', is_flag=True, help='keep as many reads of every sample as the shallowest one has')
@click.option('--seed', metavar='S', default=0, type=int, help='seed of the draw (default: 0)')
@click.option('-s', '--sample', 'samples', metavar='NAME', multiple=True, help="sample to keep, can specify multiple (default: all)")
@click.option('--samples', 'samples_file', metavar='FILE', type=click.Path(exists=True, resolve_path=True, dir_okay=False),
              help="file with the names of the samples to keep, one per line")
@click.option('-m', '--mincount', default=None, type=int, help='drop the samples that count fewer reads than this before the draw')
@click.option('--stats', 'stats_file', metavar='FILE', type=click.Path(resolve_path=True, dir_okay=False, writable=True),
              help="write sample, reads_in, reads_out, ecs_in, ecs_out per sample that stays")
@click.option('-v', '--verbose', count=True, help='enables verbose mode')
def ecdownsample(ec_file, out_file, reads, fraction, equalize, seed, samples, samples_file, mincount, stats_file, verbose):
    """
    Thin the samples of a binary EC file (ec_file) to a read depth, drawn without replacement, and write the result (out_file)
    """
    utils.configure_logging(verbose)
    try:
        methods.ecdownsample(ec_file, out_file, reads, fraction, equalize, seed, list(samples) or None, samples_file, mincount, stats_file)
    except Exception:
        sys.exit(1)                                                  # (logged as "Error: ..." by bin_utils.ecdownsample)


@cli.command('salmon2ec', options_metavar='<options>', short_help='convert a salmon eq_classes file to EC')
@click.argument('salmon_dir', metavar='salmon_dir', type=click.Path(exists=True, resolve_path=True, dir_okay=True))
@click.argument('ec_file', metavar='ec_file', type=click.Path(resolve_path=True, dir_okay=False, writable=True))
@click.option('-s', '--sample', metavar='sample', default='NA', help="sample identifier")
@click.option('-t', '--targets', metavar='FILE', type=click.Path(exists=True, resolve_path=True, file_okay=True, dir_okay=False), help="target file")
@click.option('-v', '--verbose', count=True, help='enables verbose mode')
def salmon2ec(salmon_dir, ec_file, sample, targets, verbose):
    """
    Convert a salmon eq_classes file to a binary EC file (ec_file)
    """
    utils.configure_logging(verbose)
    try:
        methods.salmon2ec(salmon_dir, ec_file, sample, targets)
    except Exception:
        sys.exit(1)                                                  # (logged as "Error: ..." by salmon_utils.convert)


@cli.command('bus2ec', options_metavar='<options>', short_help='convert a kallisto BUS directory to a multisample EC file')
@click.argument('bus_dir', metavar='bus_dir', type=click.Path(exists=True, resolve_path=True, file_okay=False, dir_okay=True))
@click.argument('ec_file', metavar='ec_file', type=click.Path(resolve_path=True, dir_okay=False, writable=True))
@click.option('--no-umi', is_flag=True, help='every record is `count` reads of its EC; UMIs are not collapsed and no intersection is taken')
@click.option('-m', '--mincount', default=1000, type=int, help='drop the cells that count fewer molecules than this (default: 1000)')
@click.option('--names', 'names_file', metavar='FILE', type=click.Path(exists=True, resolve_path=True, dir_okay=False),
              help="lines of barcode<TAB>name: the cells to keep, in this order, and their sample names (default: all, named by their sequence)")
@click.option('-l', '--lengths', 'lengths_file', metavar='FILE', type=click.Path(exists=True, resolve_path=True, dir_okay=False),
              help="lines of name<TAB>length for every target name (default: every length is 0)")
@click.option('-H', '--haplotype', metavar='NAME', default=None, help="every target name is a transcript as it stands, of this one haplotype")
@click.option('-t', '--targets', metavar='FILE', type=click.Path(exists=True, resolve_path=True, file_okay=True, dir_okay=False), help="target file")
@click.option('--stats', 'stats', metavar='FILE', default=None, type=click.Path(resolve_path=True, dir_okay=False, writable=True),
              help='write the numbers of records, molecules, new ECs and cells (with -w: and of barcodes by outcome) to this file')
@click.option('-w', '--whitelist', 'whitelist', metavar='FILE', default=None, type=click.Path(exists=True, resolve_path=True, dir_okay=False),
              help="barcode whitelist, one per line, plain or .gz: a barcode one base from exactly one of its barcodes becomes that one, "
                   "every other barcode off the list is dropped, before anything else is done (default: the barcodes are taken as they are)")
@click.option('-v', '--verbose', count=True, help='enables verbose mode')
def bus2ec(bus_dir, ec_file, no_umi, mincount, names_file, lengths_file, haplotype, targets, stats, whitelist, verbose):
    """
    Convert the output of kallisto bus (bus_dir: output.bus, matrix.ec, transcripts.txt) to a multisample binary EC file (ec_file)
    """
    utils.configure_logging(verbose)
    try:
        named = {} if whitelist is None else {"whitelist_file": whitelist}
        methods.bus2ec(bus_dir, ec_file, no_umi, mincount, names_file, lengths_file, haplotype, targets, stats, **named)
    except Exception:
        sys.exit(1)                                                  # (logged as "Error: ..." by bus_utils.convert)


@cli.command('buscorrect', options_metavar='<options>', short_help='correct the barcodes of a BUS file against a whitelist')
@click.argument('bus_file', metavar='bus_file', type=click.Path(exists=True, resolve_path=True, dir_okay=False))
@click.argument('out_file', metavar='out_file', type=click.Path(resolve_path=True, dir_okay=False, writable=True))
@click.option('-w', '--whitelist', 'whitelist', metavar='FILE', required=True, type=click.Path(exists=True, resolve_path=True, dir_okay=False),
              help="barcode whitelist, one per line, plain or .gz")
@click.option('--stats', 'stats', metavar='FILE', default=None, type=click.Path(resolve_path=True, dir_okay=False, writable=True),
              help='write the numbers of records and of barcodes by outcome to this file')
@click.option('-v', '--verbose', count=True, help='enables verbose mode')
def buscorrect(bus_file, out_file, whitelist, stats, verbose):
    """
    Write the records of a BUS file (bus_file) whose barcode is on the whitelist, or one base from exactly one of its barcodes and then
    replaced by it, behind the input's header to a BUS file (out_file), as bustools correct does
    """
    utils.configure_logging(verbose)
    try:
        methods.buscorrect(bus_file, out_file, whitelist, stats)
    except Exception:
        sys.exit(1)                                                  # (logged as "Error: ..." by bus_utils.correct_file)


@cli.command('count-alignments', options_metavar='<options>', short_help='count the alignments of an EC file per target')
@click.argument('ec_file', metavar='ec_file', type=click.Path(exists=True, resolve_path=True, dir_okay=False))
@click.argument('out_file', metavar='out_file', type=click.Path(resolve_path=True, dir_okay=False, writable=True))
@click.option('-s', '--sample', metavar='sample', default=None, help="count one sample of a multisample file (default: all of them)")
@click.option('-v', '--verbose', count=True, help='enables verbose mode')
def count_alignments(ec_file, out_file, sample, verbose):
    """
    Write the alignment, allele-unique and locus-unique read counts per target of a binary EC file (ec_file) to a table (out_file)
    """
    utils.configure_logging(verbose)
    try:
        methods.count_alignments(ec_file, out_file, sample)
    except Exception:
        sys.exit(1)                                                  # (logged as "Error: ..." by bin_utils.count_alignments)


@cli.command('ecquant', options_metavar='<options>', short_help='estimate abundances from an EC file by EM')
@click.argument('ec_file', metavar='ec_file', type=click.Path(exists=True, resolve_path=True, dir_okay=False))
@click.argument('out_file', metavar='out_file', type=click.Path(resolve_path=True, dir_okay=False, writable=True))
@click.option('-s', '--sample', metavar='sample', default=None, help="quantify one sample of a multisample file (default: all of them pooled)")
@click.option('-l', '--use-lengths', is_flag=True, help='weight every abundance by 1 / the length of its target')
@click.option('-i', '--max-iters', default=1000, type=click.IntRange(min=0), help='EM steps at the most (default: 1000)')
@click.option('-t', '--tolerance', 'tol', default=1e-6, type=float, help='stop when one step changes less than this share of the reads (default: 1e-6)')
@click.option('-M', '--model', default='4', type=click.Choice(['1', '2', '3', '4']),
              help='EMASE model: 1 gene->allele->isoform, 2 gene->isoform->allele, 3 gene->isoform x allele (each needs -g), 4 flat (default: 4)')
@click.option('-g', '--groups', metavar='<grp_file>', default=None, type=click.Path(exists=True, resolve_path=True, dir_okay=False),
              help='group file (gene, transcripts...) for models 1 to 3')
@click.option('-w', '--posterior', 'posterior', metavar='<h5_file>', default=None, type=click.Path(resolve_path=True, dir_okay=False, writable=True),
              help='also write the posterior probability of every alignment at the estimate, as an EMASE file')
@click.option('-v', '--verbose', count=True, help='enables verbose mode')
def ecquant(ec_file, out_file, sample, use_lengths, max_iters, tol, model, groups, posterior, verbose):
    """
    Estimate the abundance of every target and haplotype of a binary EC file (ec_file) by EM and write them, in reads, to a table (out_file)
    """
    utils.configure_logging(verbose)
    try:
        more = () if model == '4' and groups is None else (int(model), groups)
        named = {} if posterior is None else {"posterior_file": posterior}
        methods.ecquant(ec_file, out_file, sample, use_lengths, max_iters, tol, *more, **named)
    except Exception:
        sys.exit(1)                                                  # (logged as "Error: ..." by bin_utils.ecquant)


@cli.command('ecboot', options_metavar='<options>', short_help='bootstrap standard errors for ecquant: the reads redrawn on the GPU')
@click.argument('ec_file', metavar='ec_file', type=click.Path(exists=True, resolve_path=True, dir_okay=False))
@click.argument('out_file', metavar='out_file', type=click.Path(resolve_path=True, dir_okay=False, writable=True))
@click.option('-b', '--bootstraps', 'n_boot', required=True, type=click.IntRange(min=1), help='number of bootstrap replicates')
@click.option('--seed', default=0, type=click.IntRange(min=0, max=(1 << 64) - 1), help='seed of the resampling (default: 0)')
@click.option('-s', '--sample', metavar='sample', default=None, help="bootstrap one sample of a multisample file (default: all of them pooled)")
@click.option('-l', '--use-lengths', is_flag=True, help='weight every abundance by 1 / the length of its target')
@click.option('-i', '--max-iters', default=1000, type=click.IntRange(min=0), help='EM steps at the most, per replicate too (default: 1000)')
@click.option('-t', '--tolerance', 'tol', default=1e-6, type=float, help='stop when one step changes less than this share of the reads (default: 1e-6)')
@click.option('-M', '--model', default='4', type=click.Choice(['1', '2', '3', '4']),
              help='EMASE model: 1 gene->allele->isoform, 2 gene->isoform->allele, 3 gene->isoform x allele (each needs -g), 4 flat (default: 4)')
@click.option('-g', '--groups', metavar='<grp_file>', default=None, type=click.Path(exists=True, resolve_path=True, dir_okay=False),
              help='group file (gene, transcripts...) for models 1 to 3')
@click.option('--replicates', 'replicates', metavar='<npy_file>', default=None, type=click.Path(resolve_path=True, dir_okay=False, writable=True),
              help="also write every replicate's estimates, float64 [B, H, T], as a .npy file")
@click.option('-v', '--verbose', count=True, help='enables verbose mode')
def ecboot(ec_file, out_file, n_boot, seed, sample, use_lengths, max_iters, tol, model, groups, replicates, verbose):
    """
    Redraw the reads of a binary EC file (ec_file) n_boot times, quantify every replicate as ecquant would and write ecquant's estimate with
    the replicates' mean and standard deviation beside it to a table (out_file)
    """
    utils.configure_logging(verbose)
    try:
        methods.ecboot(ec_file, out_file, n_boot, seed, sample, use_lengths, max_iters, tol, int(model), groups, replicates)
    except Exception:
        sys.exit(1)                                                  # (logged as "Error: ..." by bin_utils.ecboot)


@cli.command('ecclusters', options_metavar='<options>', short_help='group the targets of an EC file by the reads they share')
@click.argument('ec_file', metavar='ec_file', type=click.Path(exists=True, resolve_path=True, dir_okay=False))
@click.argument('out_file', metavar='out_file', type=click.Path(resolve_path=True, dir_okay=False, writable=True))
@click.option('-s', '--sample', metavar='sample', default=None, help="weigh the ECs by one sample of a multisample file (default: all of them pooled)")
@click.option('-m', '--mincount', 'min_count', default=1, type=int, help='an EC of fewer reads than this ties nothing together (default: 1)')
@click.option('--stats', 'stats', metavar='FILE', default=None, type=click.Path(resolve_path=True, dir_okay=False, writable=True),
              help='write the targets, ECs and reads of every cluster to this file')
@click.option('--multi-only', is_flag=True, help='leave the clusters of one target out of the file')
@click.option('-v', '--verbose', count=True, help='enables verbose mode')
def ecclusters(ec_file, out_file, sample, min_count, stats, multi_only, verbose):
    """
    Group the targets of a binary EC file (ec_file) by the reads they share -- the connected components of its target-EC incidence -- and
    write them as a group file (out_file) that ecbundle and ecquant -M -g take
    """
    utils.configure_logging(verbose)
    try:
        methods.ecclusters(ec_file, out_file, sample, min_count, stats, multi_only)
    except Exception:
        sys.exit(1)                                                  # (logged as "Error: ..." by bin_utils.ecclusters)


@cli.command('ecquant-cells', options_metavar='<options>', short_help='estimate abundances per sample (cell) of a multisample EC file by EM')
@click.argument('ec_file', metavar='ec_file', type=click.Path(exists=True, resolve_path=True, dir_okay=False))
@click.argument('out_file', metavar='out_file', type=click.Path(resolve_path=True, dir_okay=False, writable=True))
@click.option('-s', '--sample', 'samples', metavar='NAME', multiple=True, help="sample to quantify, can specify multiple (default: all)")
@click.option('--samples', 'samples_file', metavar='FILE', type=click.Path(exists=True, resolve_path=True, dir_okay=False),
              help="file with the names of the samples to quantify, one per line")
@click.option('-l', '--use-lengths', is_flag=True, help='weight every abundance by 1 / the length of its target')
@click.option('-i', '--max-iters', default=1000, type=click.IntRange(min=0), help='EM steps per sample at the most (default: 1000)')
@click.option('-t', '--tolerance', 'tol', default=1e-6, type=float,
              help="stop a sample when one step changes less than this share of its reads (default: 1e-6)")
@click.option('--report', metavar='FILE', default=None, type=click.Path(resolve_path=True, dir_okay=False, writable=True),
              help='write n_iter, delta, explained and converged per sample to this file')
@click.option('-M', '--model', default='4', type=click.Choice(['1', '2', '3', '4']),
              help='EMASE model, per sample: 1 gene->allele->isoform, 2 gene->isoform->allele, 3 gene->isoform x allele (each needs -g), 4 flat (default: 4)')
@click.option('-g', '--groups', metavar='<grp_file>', default=None, type=click.Path(exists=True, resolve_path=True, dir_okay=False),
              help='group file (gene, transcripts...) for models 1 to 3')
@click.option('-v', '--verbose', count=True, help='enables verbose mode')
def ecquant_cells(ec_file, out_file, samples, samples_file, use_lengths, max_iters, tol, report, model, groups, verbose):
    """
    Estimate, for every sample of a binary EC file (ec_file), the abundance of every target it touches by an EM of its own and write them, in
    reads, to a table with one line per sample and target (out_file)
    """
    utils.configure_logging(verbose)
    try:
        more = () if model == '4' and groups is None else (int(model), groups)
        methods.ecquant_cells(ec_file, out_file, list(samples) or None, samples_file, use_lengths, max_iters, tol, report, *more)
    except Exception:
        sys.exit(1)                                                  # (logged as "Error: ..." by bin_utils.ecquant_cells)


@cli.command('ecdump', options_metavar='<options>', short_help='show the shapes of an EC file')
@click.argument('ec_file', metavar='ec_file', type=click.Path(exists=True, resolve_path=True, dir_okay=False))
@click.option('-v', '--verbose', count=True, help='enables verbose mode')
def ecdump(ec_file, verbose):
    """
    Show the number of targets, haplotypes, samples and ECs of a binary EC file (ec_file)
    """
    utils.configure_logging(verbose)
    methods.ecdump(ec_file)


if __name__ == '__main__':
    cli()
