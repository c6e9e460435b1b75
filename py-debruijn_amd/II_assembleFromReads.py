#!/usr/bin/env python3
"""Drop-in for the reference's ``II_assembleFromReads.py`` on the MI355X path.

Same CLI (``-froot``), same ``{froot}/setting.json`` keys (score_cut, k_lowerlimit,
k_upperlimit, threshold, source -- II_assembleFromReads.py:32-38; optionally non_acgt,
fold_case, reads_format, min_quality, strands and fasta_records, see ``debruijn.DeviceReads``,
fasta_line_width for the output, and spectrum_bins for a ``{froot}/{froot}_k{k}.hist`` per k), same stdout lines and
the same append-mode FASTA output ``{froot}/{froot}.fasta`` with records
``>SEQUENCE_{i}_{k}mer`` (II_assembleFromReads.py:65-69).  Input is the FASTA surface the
reference keeps commented out at II_assembleFromReads.py:53:
``sequences = read_reads(f'{froot}/input_reads.fasta')`` (the live TSV path needs the
proprietary PSM tables and is outside the hot path).

Graph construction, pruning, tip removal, pull-out reads, the contig walk and the contig
scores all run on the GPU through ``debruijn`` (this directory) -> ``include/dbg.h``.
"""
import argparse
import json

import debruijn as db
from debruijn import read_reads, read_reads_device


def getScore(edge_count_table, contig, k):
    """II_assembleFromReads.py:14-18: the counts of all (k+1)-mers of a contig, added up.  Host version of the score the
    walk kernels attach to every contig (``ContigList.scores`` / ``get_score_device``); kept for callers that import it.
    A lazy table of a large graph (debruijn.LAZY_MIN_NODES) is asked on the device: no array of the graph is exported."""
    if type(edge_count_table) is db._LazyEdgeCounts:
        return db.score_sequences(edge_count_table, [contig], k)[0]
    return sum(edge_count_table[contig[i:i + k + 1]] for i in range(len(contig) - k))


def get_args():
    parser = argparse.ArgumentParser()
    parser.add_argument('-froot', type=str)
    return parser.parse_args()


def write_spectrum(path, edge_hist):
    """The edge spectrum as lines ``count<TAB>n`` for count 1..B-1; the last line is the clamp bin (B - 1 and above)."""
    with open(path, mode='w') as out_file:
        out_file.write(''.join('{}\t{}\n'.format(c, int(edge_hist[c])) for c in range(1, len(edge_hist))))


def assemble(sequences, k_lowerlimit, k_upperlimit, threshold, out_path=None, line_width=0, spectrum_bins=0, spectrum_path=None):
    """II_assembleFromReads.py:56-75.  Returns the final, score-sorted contig list.  ``line_width`` W > 0: the contigs of
    the output file in lines of W characters (``debruijn.wrap_fasta_record``); 0: one line each, as in the reference.
    ``spectrum_bins`` B > 0: the (k+1)-mer abundance spectrum of every k's graph (``debruijn.count_spectrum``, counted on
    the device) goes to ``spectrum_path.format(k)``; nothing is printed for it."""
    for k in range(k_lowerlimit, k_upperlimit + 1):
        final = not (k <= k_upperlimit - 1)
        g, pull_out_read, branch_kmer, already_pull_out, edge_count_table = db.construct_graph(
            sequences, k, threshold=threshold, final=final)
        if spectrum_bins and spectrum_path is not None:
            write_spectrum(spectrum_path.format(k), db.count_spectrum(g, edge_count_table, spectrum_bins)["edge_hist"])
        contigs = db.output_contigs(g, branch_kmer, already_pull_out)
        if isinstance(contigs, db.LazyContigs):
            # more text than fits the host: the index is sorted (device scores == getScore), no contig text moves
            contigs.sort(reverse=True)
            sequences = contigs
            max_len = max(contigs.lengths, default=0)
        else:
            scores = db.get_score_device(contigs)  # == getScore(edge_count_table, x, k) for every contig
            order = sorted(range(len(contigs)), key=lambda i: scores[i], reverse=True)  # stable, like list.sort
            sequences = [contigs[i] for i in order]
            max_len = max((len(x) for x in sequences), default=0)
        if k == k_upperlimit:
            if out_path is not None and isinstance(sequences, db.LazyContigs):
                # append mode; formatted on the device, streamed window by window
                sequences.write_fasta(out_path, k, line_width=line_width)
            elif out_path is not None and line_width and getattr(contigs, "_graph", None) is not None:
                contigs.write_fasta(out_path, k, order, line_width=line_width)  # the score order above, wrapped on the device
            elif out_path is not None:
                with open(out_path, mode='a+') as out_file:  # append mode, as in the reference
                    if hasattr(contigs, "sorted_fasta"):
                        out_file.write(contigs.sorted_fasta())  # the same records, sorted and formatted on the device
                    else:
                        for i in range(len(sequences)):
                            out_file.write('>SEQUENCE_{}_{}mer\n{}'.format(i, k, db.wrap_fasta_record(sequences[i], line_width)))
            break
        print('max length: ', max_len)
        print('number of output for k={}: '.format(k), len(sequences))
        if k <= k_upperlimit - 1:
            sequences.extend(pull_out_read)
            print('number of pull out read: ', len(pull_out_read))
    return sequences


if __name__ == '__main__':
    args = get_args()
    froot = args.froot
    with open(f'{froot}/setting.json') as f:
        setting = json.load(f)
    k_lowerlimit = setting['k_lowerlimit']
    k_upperlimit = setting['k_upperlimit']
    threshold = setting['threshold']
    # II_assembleFromReads.py:53 with the FASTA parsed on the GPU (read_reads semantics, no Python string per read)
    # optional keys: "non_acgt": "split" cuts the reads at every byte that is not A/C/G/T, "fold_case" folds a c g t first
    # "reads_format": "fastq" reads {froot}/input_reads.fastq instead; "min_quality": q turns bases below Phred q into N
    # "strands": "both" follows every read with its reverse complement, at this ingest only: the contigs and pulled reads
    # that the later k's take already hold both strands, so nothing is doubled again
    split = {key: setting[key] for key in ('non_acgt', 'fold_case', 'min_quality', 'strands') if key in setting}
    # "fasta_records": "record" takes one read per FASTA record (a line-wrapped input file), "line" (default) one per line
    # "fasta_line_width": W writes the contigs of the output file in lines of W characters
    reads_format = setting.get('reads_format', 'fasta')
    if reads_format not in ('fasta', 'fastq'):
        raise ValueError(f"setting.json: reads_format must be 'fasta' or 'fastq', not {reads_format!r}")
    fasta_records = setting.get('fasta_records', 'line')
    if fasta_records not in ('line', 'record'):
        raise ValueError(f"setting.json: fasta_records must be 'line' or 'record', not {fasta_records!r}")
    line_width = setting.get('fasta_line_width', 0)
    if isinstance(line_width, bool) or not isinstance(line_width, int) or line_width < 0:
        raise ValueError(f"setting.json: fasta_line_width must be a non-negative integer, not {line_width!r}")
    # "spectrum_bins": B writes {froot}/{froot}_k{k}.hist for every k: the (k+1)-mer abundance spectrum of that k's graph,
    # lines "count<TAB>n" for count 1..B-1, the last line collecting every count at or above B - 1; stdout and the FASTA stay
    spectrum_bins = setting.get('spectrum_bins', 0)
    if isinstance(spectrum_bins, bool) or not isinstance(spectrum_bins, int) or spectrum_bins == 1 or not 0 <= spectrum_bins <= 1 << 20:
        raise ValueError(f"setting.json: spectrum_bins must be an integer in 2..2**20 (or 0: no spectrum), not {spectrum_bins!r}")
    if 'fasta_records' in setting:
        split['records'] = fasta_records
    sequences = read_reads_device(f'{froot}/input_reads.{reads_format}', format=reads_format, **split)
    print(len(sequences))
    assemble(sequences, k_lowerlimit, k_upperlimit, threshold, out_path=f'{froot}/{froot}.fasta', line_width=line_width,
             spectrum_bins=spectrum_bins, spectrum_path=f'{froot}/{froot}_k{{}}.hist')
