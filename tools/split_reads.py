#!/usr/bin/env python3
"""Time of the read split (dbg_split_reads, DESIGN.md "Reads cut at the bytes that are not bases") on the configs[1] image
(GPU box): N x 150 bp synthetic reads, 1.54 GB of FASTA at 10 M reads.

  ingest   file -> resident reads through the streamed ingest (dbg_set_reads_fasta_file, default chunks), page cache warm:
           the step the split follows, timed in the same session
  clean    the split of those reads: no cut byte, nothing to fold -- the pass that almost every call is
  n        1 % of the reads carry one to three N
  n+mask   the same plus a lower-case stretch of 10..100 bases in 2 % of the reads, under fold_case
  graph    the first --graph-reads reads of `n` at k = 31: build, edge order, prune, tips, pull-out reads (the device calls
           of construct_graph) as they stand -- N is a character, the generic engine; nothing on that path differs from
           the parent commit -- against split_reads + the same calls.  A smaller set runs first, and the large one is
           skipped where the small one says the generic engine would take minutes.

Times are host clocks around calls that end in a device synchronise, each the best of --reps with all of them listed.
--no-file: the reads are made on the device and the ingest is skipped (for a kernel trace of the passes alone).  Every result
is one JSON line on stdout.

    python tools/split_reads.py [--reads 10e6] [--reps 5] [--graph-reads 1e6] [--no-file] [--no-graph]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "py-debruijn_amd"))
import _dbg  # noqa: E402

L = 150


def out(**kw):
    print(json.dumps(kw), flush=True)


def ms(fn):
    t = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t) * 1e3, r


def write_file(path, bases, n):
    with open(path, "wb") as fh:
        step = 1 << 20
        for i in range(0, n, step):
            m = min(step, n - i)
            rec = np.empty((m, 3 + L + 1), dtype=np.uint8)
            rec[:, :3] = np.frombuffer(b">r\n", dtype=np.uint8)
            rec[:, 3:3 + L] = bases[i * L:(i + m) * L].reshape(m, L)
            rec[:, -1] = 10
            rec.tofile(fh)


def with_n(bases, n, rng):
    b = bases.copy()
    reads = rng.choice(n, n // 100, replace=False)
    for j in range(3):  # one to three N per chosen read
        sel = reads[rng.integers(1, 4, reads.size) > j]
        b[sel * L + rng.integers(0, L, sel.size)] = ord("N")
    return b


def with_mask(bases, n, rng):
    b = bases.copy()
    for r, s, m in zip(rng.choice(n, n // 50, replace=False), rng.integers(0, L - 10, n // 50), rng.integers(10, 101, n // 50)):
        seg = b[r * L + s:r * L + min(L, s + m)]
        seg[np.isin(seg, np.frombuffer(b"ACGT", dtype=np.uint8))] += 32
    return b


def timed_split(g, name, reps, fold, reload=None):
    times, st = [], None
    for _ in range(reps):
        if reload:
            reload()
        t, st = ms(lambda: g.split_reads(fold_case=fold))
        times.append(round(t, 3))
    out(step="split", input=name, fold_case=fold, best_ms=min(times), all_ms=times, **st)


def graph_calls(g, k):
    g.build(k)
    g.refine_edge_order()
    g.prune(2)
    g.remove_tips()
    g.mark_pull_reads()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=10e6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--graph-reads", type=float, default=1e6)
    ap.add_argument("--no-file", action="store_true")
    ap.add_argument("--no-graph", action="store_true")
    args = ap.parse_args()
    n = int(args.reads)
    off = np.arange(0, (n + 1) * L, L, dtype=np.uint64)
    g = _dbg.Graph()
    g.synth_reads(1, n * 5, n, L, 0.01)
    bases, _ = g.copy_reads()
    tmp = None
    try:
        if not args.no_file:
            tmp = tempfile.mkdtemp(prefix="split_reads_")
            path = os.path.join(tmp, "reads.fasta")
            write_file(path, bases, n)
            np.fromfile(path, dtype=np.uint8)  # warm the page cache
            times = [round(ms(lambda: g.set_reads_fasta_file(path))[0], 1) for _ in range(max(2, args.reps // 2))]
            st = g.ingest_stats()
            out(step="ingest", file_bytes=os.path.getsize(path), best_ms=min(times), all_ms=times, n_reads=st["n_reads"],
                n_bases=st["n_bases"], peak_device_bytes=st["peak_device_bytes"])
        timed_split(g, "clean", args.reps, False)
        timed_split(g, "clean", args.reps, True)
        rng = np.random.default_rng(16)
        b_n = with_n(bases, n, rng)
        timed_split(g, "n", min(args.reps, 3), False, reload=lambda: g.set_reads(b_n, off))
        b_mask = with_mask(b_n, n, rng)
        timed_split(g, "n+mask", min(args.reps, 3), True, reload=lambda: g.set_reads(b_mask, off))
        del b_mask
        if not args.no_graph:
            k, big = 31, min(n, int(args.graph_reads))
            last_keep = None
            for m in sorted({max(1, big // 10), big}):
                sub, sub_off = b_n[:m * L], off[:m + 1]
                g.set_reads(sub, sub_off)
                t_split, _ = ms(lambda: (g.split_reads(), graph_calls(g, k)))
                sz = g.sizes()
                res = {"step": "graph", "reads": m, "k": k, "split_ms": round(t_split, 1), "split_nodes": sz["n_nodes"],
                       "split_max_degree": sz["max_degree"]}
                if last_keep is not None and last_keep > 6000:
                    res["keep_ms"] = None
                    res["note"] = f"not run: the generic engine took {last_keep:.0f} ms on a tenth of these reads"
                else:
                    g.set_reads(sub, sub_off)
                    last_keep, _ = ms(lambda: graph_calls(g, k))
                    sz = g.sizes()
                    res.update(keep_ms=round(last_keep, 1), keep_nodes=sz["n_nodes"], keep_max_degree=sz["max_degree"],
                               keep_over_split=round(last_keep / t_split, 1))
                out(**res)
        g.close()
    finally:
        if tmp:
            shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
