"""Shared CLI plumbing for `mimeo self | x | map` (reference: src/mimeo/run_self.py:32-166,
run_interspecies.py:38-170, run_map.py:36-187 — same flag names, types and defaults)."""
import logging
import os
import sys

from . import engine, formats
from .dist import Dist

__version__ = '0.1.0+mi355x'


def add_common(parser, prog, gff_default, label, prefix, with_b):
    parser.add_argument('--version', action='version', version='%s %s' % (prog, __version__))
    parser.add_argument('--adir', type=str, default=None,
                        help='Directory containing sequences of genome A (one or more FASTA files).')
    if with_b:
        parser.add_argument('--bdir', type=str, default=None, help='Directory containing sequences of genome B.')
    parser.add_argument('--afasta', type=str, default=None, help='A genome as multifasta.')
    if with_b:
        parser.add_argument('--bfasta', type=str, default=None, help='B genome as multifasta.')
    parser.add_argument('-r', '--recycle', action='store_true', help='Use existing alignment "--outfile" if found.')
    parser.add_argument('-d', '--outdir', type=str, default=None, help='Write output files to this directory. (Default: cwd)')
    parser.add_argument('--gffout', type=str, default=gff_default, help='Name of GFF3 annotation file.')
    parser.add_argument('--outfile', type=str, default='mimeo_alignment.tab', help='Name of alignment result file.')
    parser.add_argument('--verbose', action='store_true', default=False, help='Report engine stage statistics.')
    parser.add_argument('--label', type=str, default=label, help='Set annotation TYPE field in gff.')
    parser.add_argument('--prefix', type=str, default=prefix, help='ID prefix for features.')
    parser.add_argument('--keeptemp', action='store_true', default=False, help='Accepted for compatibility (no temp files are made).')
    parser.add_argument('--lzpath', type=str, default='lastz', help='Accepted for compatibility; LASTZ is not used.')
    parser.add_argument('--minIdt', type=int, default=60, help='Minimum alignment identity to report.')
    parser.add_argument('--minLen', type=int, default=100, help='Minimum alignment length to report.')
    parser.add_argument('--hspthresh', type=int, default=3000, help='HSP min score threshold.')
    parser.add_argument('--loglevel', type=str, default='INFO', choices=['DEBUG', 'INFO', 'WARNING', 'ERROR', 'CRITICAL'],
                        help='Set the logging level.')
    parser.add_argument('--device', type=int, default=None, help='GPU index (default: LOCAL_RANK or 0).')
    parser.add_argument('--anchorRule', type=str, default='box', choices=['box', 'path'],
                        help='Which anchors the gapped stage skips. box (default): an anchor inside the box of an earlier '
                             'alignment of its pair and strand. path: an anchor on a match/mismatch column of the path of an '
                             'earlier alignment (lastz\'s --gapped rule); --boundExtensions adds lastz\'s bounding of a new extension by '
                             'earlier alignments. Ignored with --recycle when the alignment file exists.')
    parser.add_argument('--boundExtensions', action='store_true', default=False,
                        help='With --anchorRule path: bound every gapped extension by the earlier alignments of its pair and '
                             'strand, so that they neither cross nor run onto each other (the project\'s own statement of '
                             'lastz\'s behaviour; parity unpinned). An error without --anchorRule path.')


    parser.add_argument('--paf', type=str, default=None, metavar='FILE',
                        help='Also write the rows of the alignment file as PAF with their alignments (cg:Z: CIGAR of M/I/D, AS:i: score) '
                             'to FILE, in the same order. Off by default: without it no path is computed. Ignored with --recycle '
                             'when the alignment file exists.')
    parser.add_argument('--divergence', action='store_true', default=False,
                        help='With --paf: every PAF row also carries NM:i: (edit distance), de:f: (gap-compressed divergence), ts:i: / '
                             'tv:i: (transitions, transversions) and kd:f: (Kimura two-parameter distance; left out where undefined), '
                             'counted on the GPU from the alignment\'s columns. An error without --paf. Ignored with --recycle when the '
                             'alignment file exists.')
    parser.add_argument('--maf', type=str, default=None, metavar='FILE',
                        help='Also write the rows of the alignment file as MAF to FILE, one block per row in the same order: the '
                             'alignment itself as text, target over query, made on the GPU from the resident genomes. The letters are '
                             'A C G T in upper case and N for everything else: the engine keeps neither case nor IUPAC codes, so a '
                             'soft-masked a is written A, and R or n is written N. Does not need --paf. Nothing is written with '
                             '--recycle when the alignment file exists.')
    parser.add_argument('--cs', action='store_true', default=False,
                        help='With --paf: every PAF row also carries minimap2\'s short cs:Z: tag behind cg:Z: (:n matches, *xy a '
                             'substitution or a column with an n, +seq / -seq inserted and deleted bases; target as the reference, lower '
                             'case, n for everything that is not ACGT). An error without --paf.')


def add_region_stats(parser):
    """--regionStats of `mimeo self` and `mimeo x` (`mimeo map` has no regions)"""
    parser.add_argument('--regionStats', type=str, default=None, metavar='FILE',
                        help='Also write one line per feature of the GFF3 to FILE (tab-separated, with a header): the alignment rows that '
                             'overlap the region, and the matches, transitions, transversions, ambiguous columns and insertion / deletion '
                             'runs and bases of their alignments clipped to the region, counted on the GPU, with identity, gap-compressed '
                             'divergence (de) and Kimura two-parameter distance (kd) over the region; "." where undefined. The trivial '
                             'alignment of a scaffold with itself is left out. Needs neither --paf nor --divergence. Nothing is written '
                             'with --recycle when the alignment file exists.')


def add_families(parser):
    """--families / --familyCover of `mimeo self` (`mimeo x` has its query in another genome)"""
    parser.add_argument('--families', type=str, default=None, metavar='FILE',
                        help='Also write one line per feature of the GFF3 to FILE (tab-separated, with a header): its ID, seqid, start and '
                             'end, the repeat family it belongs to (F1, F2, ... in the order of their first member; with --strictSelf the '
                             'same-scaffold block follows as F1_intra, ...), the members and summed bases of the family, and how often '
                             'the feature was linked to another one. Two features are of one family when an alignment row that covers '
                             '--familyCover per cent of the one lands, through its alignment, on --familyCover per cent of the other; '
                             'computed on the GPU. Off by default: without it no path is computed. Nothing is written with --recycle when '
                             'the alignment file exists.')
    parser.add_argument('--familyCover', type=int, default=80, metavar='PCT',
                        help='With --families: the share of a feature, in per cent (1..100), that an alignment must cover on both '
                             'sides to link two features. Default 80, the "80 %% of the length" of the 80-80-80 rule for transposable-'
                             'element families; identity is governed by --minIdt.')


def add_consensus(parser):
    """--consensus of `mimeo self` (`mimeo x` has its query in another genome; `mimeo map` and `mimeo filter` read a library)"""
    parser.add_argument('--consensus', type=str, default=None, metavar='FILE',
                        help='Also write a repeat library to FILE: one FASTA record per repeat family (the families of --families, which '
                             'need not be given; --familyCover applies), named F1, F2, ... (with --strictSelf the same-scaffold block '
                             'follows as F1_intra, ...). The sequence is the consensus of the alignments that pile up on the family\'s '
                             'representative feature, called column by column on the GPU; the header names the feature, its position, '
                             'the members of the family, the mean depth of the pile and the columns at which most copies carry an '
                             'insertion (which the consensus leaves out). Ready for mimeo filter and mimeo map. Off by default: without '
                             'it no path is computed. Nothing is written with --recycle when the alignment file exists.')
    parser.add_argument('--consensusInsertions', action='store_true',
                        help='With --consensus: where most copies carry an insertion in front of a column of the representative feature, '
                             'pile up the inserted bases too and call them on the GPU, and put them into the record, so that a deletion '
                             'private to the representative does not become the family\'s. The header then also reports inserted=<bases>. '
                             'Every other output is unchanged. Off by default.')


def add_family_alignments(parser):
    """--familyAlignments of `mimeo self` (`mimeo x` has its query in another genome)"""
    parser.add_argument('--familyAlignments', type=str, default=None, metavar='FILE',
                        help='Also write the evidence behind the repeat library to FILE: one Stockholm 1.0 block per repeat family (the '
                             'families of --families; --familyCover applies; neither --families nor --consensus need be given), named '
                             'F1, F2, ... (with --strictSelf the same-scaffold block follows as F1_intra, ...). A block holds the '
                             'representative feature\'s own row and one row per alignment that piles up on it, named '
                             '<seqid>/<start>-<end> (start > end on the minus strand), in the representative\'s coordinates with the '
                             'columns that copies insert opened up (lower case), the #=GC RF line marking the representative\'s columns '
                             'and #=GC cons the consensus of --consensus --consensusInsertions. The rows are made on the GPU. Ready for '
                             'a profile-HMM builder. Off by default. Nothing is written with --recycle when the alignment file exists.')


def add_copy_divergence(parser):
    """--copyDivergence and --landscape of `mimeo self` (`mimeo x` has its query in another genome)"""
    parser.add_argument('--copyDivergence', type=str, default=None, metavar='FILE',
                        help='Also write to FILE, tab-separated, one line per member of every repeat family (the families of --families; '
                             '--familyCover applies; none of --families, --consensus, --familyAlignments need be given): the '
                             'representative feature (role rep) and every copy that aligns to it (role copy; the sequence rows of '
                             '--familyAlignments), with the copy\'s position, its columns against the family\'s consensus (that of '
                             '--consensus --consensusInsertions) counted on the GPU - matches, transitions, transversions, ambiguous, '
                             'ins_bases, del_bases - the divergence (ts + tv) / (m + ts + tv) and Kimura\'s two-parameter distance kd, '
                             'which dates the copy. Off by default. Nothing is written with --recycle when the alignment file exists.')
    parser.add_argument('--landscape', type=str, default=None, metavar='FILE',
                        help='Also write the repeat landscape to FILE, tab-separated: per repeat family, and over all of them (family '
                             '"all"), the members of --copyDivergence binned by their Kimura distance to the family\'s consensus in bins of '
                             '0.01 up to 0.50 (then 0.50-inf, and NA for saturated copies), with the copies and the aligned bases in each '
                             'non-empty bin. Works alone or with --copyDivergence, which shares its computation. Off by default. '
                             'Nothing is written with --recycle when the alignment file exists.')


def add_terminal_repeats(parser):
    """--terminalRepeats, --terminalWindow and --terminalMinScore of `mimeo self` (the features of `mimeo x` lie in another genome)"""
    parser.add_argument('--terminalRepeats', type=str, default=None, metavar='FILE',
                        help='Also write to FILE, tab-separated, the repeats at the two ends of every feature of the GFF3: its first '
                             '--terminalWindow bases against its last, as they are (kind LTR: a direct repeat, the long terminal repeats of '
                             'a retrotransposon; kd between the two dates the insertion) and against their reverse complement (kind TIR: '
                             'the terminal inverted repeats of a DNA transposon). An exhaustive affine-gap local alignment on the GPU '
                             '(match 2, mismatch 3, gap open 5, gap extend 2), with no seed and none of --minIdt / --minLen, so a TIR of 20 '
                             'bases is found. One line per orientation found: position of both repeats, score, columns, matches, '
                             'transitions, transversions, gaps, identity, kd. Needs none of --paf, --families, --consensus. Off by default.')
    parser.add_argument('--terminalWindow', type=int, default=1024, metavar='N',
                        help='Bases of each end of a feature that --terminalRepeats examines, at most half the feature (1..4096). Default: 1024')
    parser.add_argument('--terminalMinScore', type=int, default=40, metavar='S',
                        help='Lowest score that --terminalRepeats reports. Two random 1024-base windows reached 19..25 (12 draws; 13..23 at '
                             '256 bases, 40 draws), so the default keeps chance out while a perfect 20-base repeat (score 40) passes. Default: 40')


def check_terminal(parser, args):
    """the ranges of --terminalWindow and --terminalMinScore (parser.error exits with status 2, before the engine starts)"""
    if not 1 <= args.terminalWindow <= 4096:
        parser.error('--terminalWindow must be in 1..4096')
    if args.terminalMinScore < 1:
        parser.error('--terminalMinScore must be at least 1')
    return args


def add_elements(parser):
    """--elements and its parameters of `mimeo self` (the features of `mimeo x` lie in another genome)"""
    parser.add_argument('--elements', type=str, default=None, metavar='FILE',
                        help='Also write to FILE, tab-separated, one structural line per feature of the GFF3: the terminal repeats of '
                             '--terminalRepeats (kind LTR or TIR; --terminalWindow and --terminalMinScore apply, --terminalRepeats need not be '
                             'given), the target-site duplication (TSD) immediately outside them - the short direct repeat of host sequence '
                             'that the insertion made, which fixes the element\'s first and last base (el_start, el_end) - the longest open '
                             'reading frame inside the element over its six frames, and a class: LTR_retrotransposon, LTR_nonautonomous, '
                             'LTR_candidate (no TSD), DNA_transposon, MITE (a non-coding TIR element of at most 800 bases), '
                             'DNA_nonautonomous, TIR_candidate (no TSD), coding_repeat. TSDs and frames are found on the GPU. With --tsdMismatch '
                             '0 a random site has at most (2*tsdSlack+1)^2 * 4^-tsdMin * 4/3 chance candidates, 0.13 at the defaults '
                             '(derived; 0.073 of 2000 random sites had one in a restatement): a 4-base TSD is weak evidence, a 6-base one strong - '
                             'the file reports tsd_len. Off by default.')
    parser.add_argument('--tsdMin', type=int, default=4, metavar='N', help='Shortest TSD that --elements reports, after 3 bases are charged per mismatch (2..32). Default: 4')
    parser.add_argument('--tsdMax', type=int, default=20, metavar='N', help='Longest TSD that --elements looks for (tsdMin..32). Default: 20')
    parser.add_argument('--tsdSlack', type=int, default=2, metavar='N',
                        help='Bases by which either end of the terminal-repeat pair may move to meet the TSD (0..8). Default: 2')
    parser.add_argument('--tsdMismatch', type=int, default=0, metavar='N', help='Mismatches allowed inside a TSD, never in its end columns (0..2). Default: 0')
    parser.add_argument('--elementMinOrf', type=int, default=300, metavar='CODONS',
                        help='Codons from which the longest open frame makes an element coding for the class of --elements. A random open run '
                             'reaches 300 codons with probability (61/64)^300, about 6e-7 per start; at 100 codons it is 0.8 per cent. Default: 300')


def check_elements(parser, args):
    """the ranges of --tsdMin, --tsdMax, --tsdSlack, --tsdMismatch and --elementMinOrf (parser.error exits with status 2, before
    the engine starts)"""
    if not 2 <= args.tsdMin <= 32:
        parser.error('--tsdMin must be in 2..32')
    if not args.tsdMin <= args.tsdMax <= 32:
        parser.error('--tsdMax must be in tsdMin..32')
    if not 0 <= args.tsdSlack <= 8:
        parser.error('--tsdSlack must be in 0..8')
    if not 0 <= args.tsdMismatch <= 2:
        parser.error('--tsdMismatch must be in 0..2')
    if args.elementMinOrf < 1:
        parser.error('--elementMinOrf must be at least 1')
    return args


def check_consensus(parser, args):
    """--consensusInsertions of `mimeo self` (parser.error exits with status 2, before the engine starts)"""
    if args.consensusInsertions and args.consensus is None:
        parser.error('--consensusInsertions needs --consensus')
    return args


def check_families(parser, args):
    """--familyCover of `mimeo self` (parser.error exits with status 2, before the engine starts)"""
    if not 1 <= args.familyCover <= 100:
        parser.error('--familyCover must be in 1..100')
    return args


def check_common(parser, args):
    """cross-flag rules of add_common (parser.error exits with status 2)"""
    if args.boundExtensions and args.anchorRule != 'path':
        parser.error('--boundExtensions needs --anchorRule path')
    if args.divergence and not args.paf:
        parser.error('--divergence needs --paf')
    if args.cs and not args.paf:
        parser.error('--cs needs --paf')
    return args


TMAXPERIOD_MAX = 2000   # TRF's own upper end for its maxperiod argument; the tandem scorer (K8) takes 1 .. 2000


def check_tmaxperiod(parser, args):
    """--tmaxperiod of `mimeo map` and `mimeo filter` (parser.error exits with status 2, before the engine starts)"""
    if not 1 <= args.tmaxperiod <= TMAXPERIOD_MAX:
        parser.error('--tmaxperiod must be in 1..%d' % TMAXPERIOD_MAX)
    return args


def init_logging(level):
    logging.basicConfig(level=getattr(logging, level), format='%(asctime)s %(levelname)s %(message)s', stream=sys.stderr)


def load_genome(fasta, directory, what):
    """utils.py:339-469 set_paths + :274-309 splitFasta: the genome is streamed from disk straight to
    the device by the native parser (engine.Genome.from_fasta).  As in the reference, a multi-FASTA
    given together with --adir/--bdir is also split into `<dir>/<id>.fa`; a directory alone is read
    file by file (sorted order)."""
    split_dir = None
    if fasta:
        if not os.path.isfile(fasta):
            logging.error('%s-genome fasta not found at path: %s' % (what, fasta))
            sys.exit(1)
        paths = [fasta]
        if directory:
            split_dir = os.path.abspath(directory)
            if not os.path.isdir(split_dir):
                logging.info('Creating %sdir: %s' % (what, split_dir))
                os.makedirs(split_dir, exist_ok=True)
    elif directory and os.path.isdir(directory):
        paths = [os.path.join(directory, fn) for fn in sorted(os.listdir(directory))
                 if os.path.isfile(os.path.join(directory, fn))]
    else:
        logging.error('No %s-genome fasta file provided. Quitting.' % what)
        sys.exit(1)
    try:
        G = engine.Genome.from_fasta(paths, split_dir if Dist().rank == 0 else None)
    except RuntimeError as e:
        if 'Non-unique name' in str(e):  # utils.py:300-306
            logging.error(str(e))
            sys.exit(1)
        raise
    if not G.names:
        logging.error('No sequences found for genome %s \n Cannot calculate seq lengths.' % what)
        sys.exit(1)
    return G


def start(args):
    init_logging(args.loglevel)
    dist = Dist().init()
    dev = args.device if args.device is not None else int(os.environ.get('MIMEO_FORCE_DEVICE', dist.local_rank))
    engine.init(dev)
    outdir = os.path.abspath(args.outdir) if args.outdir else os.getcwd()
    if dist.rank == 0 and not os.path.isdir(outdir):
        logging.info('Create output directory: %s' % outdir)
        os.makedirs(outdir)
    dist.barrier()
    return dist, outdir
