#!/usr/bin/env python3
"""Time of the final-mode walk over a graph in PARTS (part_traversal.walk_final over dbg_part_final_walk)
against dbg_walk(final) on the same reads as ONE graph.

Input: synthetic reads (synth seed 1) -- by default the 3 k x 100 bp over 30 kbp of tests/test_part_final_walk.py at
k = 40 with 0.2 % errors; --genome 100000 --reads 10000 --k 21 is BASELINE configs[0].  Steps, each the best of --repeat:

  parts   build_multipass in --passes parts, prune, pull-out scan, tips (not timed), then walk_final: entries, segments,
          ranking, the contracted graph and the library's walk; the library call alone is reported beside it
  single  build, refine_edge_order, prune, tips (not timed), then dbg_walk(final) with the same max_chars

The single-graph walk has no step budget, so it only runs where the walk in parts finished within its own
(option "part_final_walk_steps") and within --max-chars; a refusal is reported and ends the run.
usage: part_final_walk.py [--genome N] [--reads N] [--read-len L] [--err E] [--k K] [--threshold T] [--passes P]
                          [--max-chars C] [--repeat R]
Every result is one JSON line on stdout."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def out(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return time.perf_counter() - t, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=30_000)
    ap.add_argument("--reads", type=int, default=3_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--err", type=float, default=0.002)
    ap.add_argument("--k", type=int, default=40)
    ap.add_argument("--threshold", type=float, default=2)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--max-chars", type=int, default=1 << 30)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "py-debruijn_amd"))
    import numpy as np
    import _dbg
    import part_traversal

    g = _dbg.Graph()
    g.synth_reads(1, args.genome, args.reads, args.read_len, args.err)
    g.build_multipass(args.k, args.passes)
    t = part_traversal.PartTraversal(g, args.k)
    branch = t.prune(args.threshold)
    t.pull_out_reads()
    pulled = t.remove_tips()
    lib_s = []
    real = g.part_final_walk

    def timing(*a, **kw):
        s, r = timed(lambda: real(*a, **kw))
        lib_s.append(s)
        return r
    g.part_final_walk = timing
    best, index = None, None
    t_first = time.perf_counter()
    try:
        for _ in range(args.repeat):
            s, index = timed(lambda: t.walk_final(max_chars=args.max_chars))
            best = s if best is None else min(best, s)
    except _dbg.DbgError as e:
        out(step="parts", refused=str(e), sizes=getattr(e, "sizes", None), n_branch=int(branch["gid"].size), passes=args.passes,
            seconds_since_first_call=round(time.perf_counter() - t_first, 3))
        g.close()
        return
    del g.part_final_walk
    pieces = None if t.final is None else int(t.final["piece_row"].size)
    out(step="parts", passes=args.passes, k=args.k, reads=args.reads, err=args.err, n_nodes=int(sum(t.n_nodes)),
        n_branch=int(branch["gid"].size), n_pulled=int(pulled["gid"].size), n_contigs=int(index["length"].size),
        contig_chars=int(index["length"].sum()), n_pieces=pieces, walk_final_s=round(best, 5),
        library_call_s=round(min(lib_s), 5) if lib_s else None)
    want = (index["stamp"], index["seq"], index["length"], index["score"])
    g.close()

    g = _dbg.Graph()
    g.synth_reads(1, args.genome, args.reads, args.read_len, args.err)
    g.build(args.k)
    g.refine_edge_order()
    g.prune(args.threshold)
    g.remove_tips()
    best = min(timed(lambda: g.walk(1, args.max_chars))[0] for _ in range(args.repeat))
    off, score, stamp, seq = g.export_contig_index()
    order = np.lexsort((seq, stamp))
    got = (stamp[order], seq[order], (off[1:] - off[:-1])[order].astype(np.int64), score[order].astype(np.int64))
    out(step="single", n_nodes=g.sizes()["n_nodes"], n_contigs=int(order.size), contig_chars=int(got[2].sum()), walk_s=round(best, 5),
        same_index=all(np.array_equal(a, b) for a, b in zip(got, want)))
    g.close()


if __name__ == "__main__":
    main()
