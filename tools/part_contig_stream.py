#!/usr/bin/env python3
"""Cost of bringing contig text off a graph in PARTS: PartContigs.texts / packed / write_fasta, the one-off
cost of handing the ranked skeleton to the library, and the single-graph export of the same contigs as the yardstick.

Input: that of tools/contig_stream.py -- the first 1 M reads of BASELINE configs[1] (synth seed 1, 50 Mbp genome, 150 bp,
1 % errors), k = 31, threshold 2, non-final -- built in 4 parts on one handle.  One process; steps:

  skeleton  part_set_skeleton again with the columns the walk handed over: copy, validation, lifting table (best of 3)
  texts     PartContigs.texts(all): one str per contig at the end
  packed    PartContigs.packed()
  writer    write_fasta in the driver's order to a tmpfs path at 4, 16 and 64 MiB windows, with the stats of every call
  single    the same reads as ONE graph, index-only walk, export_contig_texts of all contigs (tools/contig_stream.py
            "batched all"), and whether the two texts are equal

With --pkg DIR the package and library of another checkout -- the parent commit, built -- run what they have: texts, on a
random sample of --sample contigs where --sample is given (the per-piece path makes one kernel call per part and one host
copy per piece).  usage: part_contig_stream.py [--steps ...] [--pkg DIR] [--sample N] [--reads N] [--passes P]
Every result is one JSON line on stdout."""
import argparse
import hashlib
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
    ap.add_argument("--steps", default="skeleton,texts,packed,writer,single")
    ap.add_argument("--pkg", default=None, help="root of another checkout whose package and library run instead")
    ap.add_argument("--sample", type=int, default=0, help="texts: this many random contigs instead of all")
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--passes", type=int, default=4)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.pkg or ROOT, "py-debruijn_amd"))
    import numpy as np
    import _dbg
    import part_traversal
    label = "parent" if args.pkg else "this"
    steps = args.steps.split(",")

    g = _dbg.Graph()
    g.synth_reads(SEED, GENOME, args.reads, READ_LEN, ERR)
    s_build, _ = timed(lambda: g.build_multipass(K, args.passes))
    cols = []
    if hasattr(g, "part_set_skeleton"):
        real = g.part_set_skeleton
        g.part_set_skeleton = lambda *c: (cols.extend(c), real(*c))[1]
    t, _, _, _ = part_traversal.construct_graph(g, K, THRESHOLD)
    s_walk, ctg = timed(lambda: part_traversal.output_contigs(t))
    if cols:
        del g.part_set_skeleton
    n = len(ctg)
    out(step="graph", pkg=label, passes=args.passes, part_nodes=[g.part_sizes(p)["n_nodes"] for p in range(args.passes)], n_contigs=n,
        contig_chars=int(ctg.lengths.sum()), longest=int(ctg.lengths.max()), skeleton_rows=int(cols[0].numel()) if cols else None,
        build_s=round(s_build, 3), walk_s=round(s_walk, 3))
    tmp = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else tempfile.gettempdir()
    path = os.path.join(tmp, f"part_contig_stream_{os.getpid()}.fasta")

    if "skeleton" in steps and cols:
        best = min(timed(lambda: g.part_set_skeleton(*cols))[0] for _ in range(3))
        g.part_export_contig_texts(t.skeleton["emit"][:1])
        st = g.contig_output_stats()
        rows = int(cols[0].numel())
        out(step="skeleton", pkg=label, rows=rows, seconds=round(best, 5), lift_bytes=st["lift_bytes"], levels=st["lift_bytes"] // (4 * rows),
            copy_bytes=26 * rows)

    sha_parts = None
    if "texts" in steps:
        which = np.arange(n) if not args.sample else np.sort(np.random.default_rng(11).choice(n, size=min(args.sample, n), replace=False))
        s, texts = timed(lambda: ctg.texts(which.tolist()))
        h = hashlib.sha1("".join(texts).encode("ascii")).hexdigest()
        if not args.sample:
            sha_parts = h
        out(step="texts", pkg=label, contigs=len(texts), chars=sum(map(len, texts)), seconds=round(s, 4),
            us_per_contig=round(1e6 * s / max(len(texts), 1), 3), sha1=h[:16])
        del texts

    if "packed" in steps and hasattr(ctg, "packed"):
        s, (chars, off) = timed(ctg.packed)
        sha_parts = hashlib.sha1(chars.tobytes()).hexdigest()
        out(step="packed", pkg=label, contigs=n, chars=int(chars.size), seconds=round(s, 4), us_per_contig=round(1e6 * s / n, 3),
            sha1=sha_parts[:16], stats=g.contig_output_stats())
        del chars

    if "writer" in steps and hasattr(ctg, "write_fasta"):
        for chunk in (4 * MIB, 16 * MIB, 64 * MIB):
            s, nbytes = timed(lambda: t.write_contigs_fasta(path, None, k_label=K, append=False, chunk_bytes=chunk))
            out(step="writer", pkg=label, chunk_mib=chunk // MIB, bytes=nbytes, seconds=round(s, 4), gb_per_s=round(nbytes / s / 1e9, 3),
                stats=g.contig_output_stats())
        os.unlink(path)
    g.close()

    if "single" in steps and not args.pkg:
        g = _dbg.Graph()
        g.set_option("walk_jump_min_nodes", 1)
        g.synth_reads(SEED, GENOME, args.reads, READ_LEN, ERR)
        g.build(K)
        g.refine_edge_order()
        g.prune(THRESHOLD)
        g.remove_tips()
        g.mark_pull_reads()
        g.walk(False, 1)
        off, score, stamp, seq = g.export_contig_index()
        order = np.lexsort((seq, stamp))            # dict order of the starts: the order of the contigs in parts
        g.export_contig_text(0, int(off[1] - off[0]))  # the lifting tables are built once per walk: not part of the figure
        best, sha = None, None
        for _ in range(3):
            s, (o, chars) = timed(lambda: g.export_contig_texts(order))
            best = s if best is None else min(best, s)
            sha = hashlib.sha1(chars.tobytes()).hexdigest()
        out(step="single", contigs=int(order.size), chars=int(chars.size), seconds=round(best, 4), sha1=sha[:16],
            equal_to_parts=None if sha_parts is None else sha == sha_parts, stats=g.contig_output_stats())
        g.close()


if __name__ == "__main__":
    main()
