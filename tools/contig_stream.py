#!/usr/bin/env python3
"""Cost of bringing contig text off the device after a walk that kept only its index: one call per contig against the
batched export and the streamed FASTA writer.

Input: the first 1 M reads of BASELINE configs[1] (synth seed 1, 50 Mbp genome, 150 bp, 1 % errors), k = 31, threshold 2,
non-final, walked with max_chars 1 (forced index-only): 611 279 contigs, 6.8e7 characters.  One process, one graph; steps:

  loop     dbg_export_contig_text for a fixed random sample of the contigs, one call each (what every caller did before)
  batched  export_contig_texts for the same sample and for all contigs
  writer   write_contigs_fasta of all contigs in the driver's order to a tmpfs path at 4, 16 and 64 MiB windows, with the
           stats of every call
  driver   the driver's last step: LazyContigs.sort(reverse=True) and the file write of II_assembleFromReads.assemble
           (write_fasta where the package has it, else the record-by-record loop it replaced)

With --pkg DIR the package and library of another checkout -- the parent commit, built -- run the steps they have
(loop, driver).  usage: contig_stream.py [--steps loop,batched,writer,driver] [--pkg DIR] [--sample N] [--reads N]
Every result is one JSON line on stdout."""
import argparse
import contextlib
import hashlib
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, GENOME, READ_LEN, ERR, K, THRESHOLD = 1, 50_000_000, 150, 0.01, 31, 2
MIB = 1 << 20


def out(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return time.perf_counter() - t, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="loop,batched,writer,driver")
    ap.add_argument("--pkg", default=None, help="root of another checkout whose package and library run instead")
    ap.add_argument("--sample", type=int, default=50_000)
    ap.add_argument("--reads", type=int, default=1_000_000)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.pkg or ROOT, "py-debruijn_amd"))
    import numpy as np
    import _dbg
    import debruijn
    label = "parent" if args.pkg else "this"
    steps = args.steps.split(",")

    g = _dbg.Graph()
    g.set_option("walk_jump_min_nodes", 1)
    g.synth_reads(SEED, GENOME, args.reads, READ_LEN, ERR)
    g.build(K)
    g.refine_edge_order()
    g.prune(THRESHOLD)
    g.remove_tips()
    g.mark_pull_reads()
    g.walk(False, 1)
    sz = g.sizes()
    assert sz["contigs_materialised"] == 0
    off, score, stamp, seq = g.export_contig_index()
    lengths = np.diff(off.astype(np.int64))
    n = len(lengths)
    out(step="graph", pkg=label, n_nodes=sz["n_nodes"], n_contigs=n, contig_chars=int(lengths.sum()), longest=int(lengths.max()))
    sample = np.random.default_rng(11).choice(n, size=min(args.sample, n), replace=False)
    tmp = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else tempfile.gettempdir()
    path = os.path.join(tmp, f"contig_stream_{os.getpid()}.fasta")
    g.export_contig_text(0, int(lengths[0]))  # the lifting tables are built once per walk: not part of any figure below

    sha = None
    if "loop" in steps:
        def loop():
            h = hashlib.sha1()
            for i in sample.tolist():
                h.update(g.export_contig_text(i, int(lengths[i])))
            return h.hexdigest()
        s, sha = timed(loop)
        out(step="loop", pkg=label, contigs=len(sample), chars=int(lengths[sample].sum()), seconds=round(s, 4),
            us_per_contig=round(1e6 * s / len(sample), 2), sha1=sha[:16])

    if "batched" in steps and hasattr(g, "export_contig_texts"):
        s, (o, chars) = timed(lambda: g.export_contig_texts(sample))
        got = hashlib.sha1(chars.tobytes()).hexdigest()
        out(step="batched", pkg=label, what="sample", contigs=len(sample), chars=int(chars.size), seconds=round(s, 4),
            us_per_contig=round(1e6 * s / len(sample), 3), sha1=got[:16], equal_to_loop=None if sha is None else got == sha,
            stats=g.contig_output_stats())
        s, (o, chars) = timed(lambda: g.export_contig_texts(np.arange(n)))
        out(step="batched", pkg=label, what="all", contigs=n, chars=int(chars.size), seconds=round(s, 4),
            us_per_contig=round(1e6 * s / n, 3), stats=g.contig_output_stats())
        del chars

    if "writer" in steps and hasattr(g, "write_contigs_fasta"):
        for chunk in (4 * MIB, 16 * MIB, 64 * MIB):
            s, nbytes = timed(lambda: g.write_contigs_fasta(path, None, append=False, chunk_bytes=chunk))
            out(step="writer", pkg=label, chunk_mib=chunk // MIB, bytes=nbytes, seconds=round(s, 4),
                gb_per_s=round(nbytes / s / 1e9, 3), stats=g.contig_output_stats())
        os.unlink(path)

    if "driver" in steps:
        lazy = debruijn.LazyContigs(g, np.lexsort((seq, stamp)), off, score)
        lazy._final, lazy._generation, lazy._walk = False, g.generation, g.walks

        def last_step():
            lazy.sort(reverse=True)
            if hasattr(lazy, "write_fasta"):
                lazy.write_fasta(path, K)
            else:  # II_assembleFromReads.assemble before the streamed writer
                with open(path, mode="a+") as out_file:
                    for i in range(len(lazy)):
                        out_file.write(">SEQUENCE_{}_{}mer\n{}\n".format(i, K, lazy[i]))
        with contextlib.redirect_stdout(io.StringIO()):
            s, _ = timed(last_step)
        h = hashlib.sha1()
        with open(path, "rb") as fh:
            for block in iter(lambda: fh.read(1 << 24), b""):
                h.update(block)
        out(step="driver", pkg=label, contigs=n, bytes=os.path.getsize(path), seconds=round(s, 3), sha1=h.hexdigest()[:16])
        os.unlink(path)
    g.close()


if __name__ == "__main__":
    main()
