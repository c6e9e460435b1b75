#!/usr/bin/env python3
"""Rates of the query side (dbg_lookup_nodes, dbg_score_sequences, the lazy views of debruijn.py) at two sizes:

  bench   10 M x 150 bp synthetic reads, k = 31 (the flagship build of bench.py)
  k63     1 M x 150 bp, k = 63 (two-word keys)

Steps, each in a child process under its own time limit; the tool stops at the first step that fails:

  view     the first `kmer in vertices` through the views of debruijn.py, built over the handle the way construct_graph
           builds them (reads generated on the device; refine, prune, tips first).  With --pkg DIR the package of another
           checkout -- the parent commit, built -- answers instead: its first lookup exports every array and sorts the
           keys on the host.
  lookup   lookup_nodes of 1e7 present and 1e7 absent keys, host arrays and device tensors, through the build's directory
           and with "lookup_index" 1 (the sort that builds the index is reported by itself)
  score    score_sequences over 1e5 substrings of the genome of 1 000 characters each, against the host getScore loop
           (the loaded views, one searchsorted per window) on a 100-sequence sample

usage: lookup_rate.py [--sizes bench,k63] [--steps view,lookup,score] [--pkg DIR] [--no-host-loop] [--limit SECONDS]
Every result is one JSON line on stdout."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"bench": dict(n=10_000_000, glen=50_000_000, err=0.01, k=31), "k63": dict(n=1_000_000, glen=5_000_000, err=0.01, k=63)}
READ_LEN, SEED = 150, 1


def out(**kw):
    print(json.dumps(kw), flush=True)


def graph_for(size, traverse):
    import _dbg
    c = SIZES[size]
    g = _dbg.Graph()
    g.synth_reads(SEED, c["glen"], c["n"], READ_LEN, c["err"])
    g.build(c["k"])
    if traverse:
        g.refine_edge_order()
        g.prune(3)
        g.remove_tips()
    return g, c


def views_over(g, k):
    """(vertices, edges, edge_count_table) as construct_graph hands them out above LAZY_MIN_NODES."""
    import numpy as np
    import debruijn
    alphabet, bits = g.alphabet()
    two_words = bits * k > 64

    def load_arrays():
        keys, stamps, counts, flags = g.export_nodes()
        rank_mc, rank_fs = g.export_orders()
        return {"keys": keys, "stamps": stamps, "counts": counts, "flags": flags, "rank_mc": rank_mc, "rank_fs": rank_fs,
                "order": g.export_dict_order().astype(np.int64), "keys_hi": g.export_keys_hi() if two_words else None,
                "keep": g.export_keepmask()}

    n = g.sizes()["n_nodes"]
    try:
        store = debruijn._NodeStore(k, alphabet, bits, n, load_arrays, graph=g)
    except TypeError:  # a checkout from before the query calls
        store = debruijn._NodeStore(k, alphabet, bits, n, load_arrays)
    return debruijn._LazyVertices(store), debruijn._LazyEdges(store), debruijn._LazyEdgeCounts(store)


def genome_text(c, start, length):
    import numpy as np
    import synth
    return synth.ALPHABET[synth.genome_codes(SEED, start, length).astype(np.intp)].tobytes()


def step_view(size, args):
    g, c = graph_for(size, True)
    V, E, ect = views_over(g, c["k"])
    chars, _ = g.take_reads([0])
    kmer = chars[:c["k"]].tobytes().decode()
    t = time.perf_counter()
    found = kmer in V
    first = time.perf_counter() - t
    t = time.perf_counter()
    for _ in range(100):
        found = (kmer in V) and found
    later = (time.perf_counter() - t) / 100
    out(step="view", size=size, pkg=args.pkg or "this", n_nodes=g.sizes()["n_nodes"], found=bool(found),
        first_lookup_s=round(first, 6), later_lookup_s=round(later, 6), arrays_loaded=V._s._arrays is not None)


def step_lookup(size, args):
    import numpy as np
    import torch
    g, c = graph_for(size, False)
    k, n_nodes, nq = c["k"], g.sizes()["n_nodes"], 10_000_000
    rng = np.random.default_rng(7)
    rows = g.gather_nodes(rng.integers(0, n_nodes, nq), what=("keys", "keys_hi"))
    present = (rows["keys_hi"], rows["keys"])
    width = 2 * k
    absent = (rng.integers(0, 1 << 64, nq, dtype=np.uint64) & np.uint64(((1 << width) - 1) >> 64),
              rng.integers(0, 1 << 64, nq, dtype=np.uint64) & np.uint64(((1 << width) - 1) & ((1 << 64) - 1)))
    dev = torch.device("cuda", g.sizes_device())

    def timed(fn, reps=3):
        best = None
        for _ in range(reps):
            torch.cuda.synchronize(dev)
            t = time.perf_counter()
            r = fn()
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t
            best = dt if best is None else min(best, dt)
        return best, r

    for path in ("directory", "index"):
        g.set_option("lookup_index", 1 if path == "index" else 0)
        before = g.stats()
        if path == "index":
            t = time.perf_counter()
            g.lookup_nodes(present[1][:1], present[0][:1])
            out(step="lookup", size=size, path=path, what="first call (builds the index)", n_nodes=n_nodes,
                seconds=round(time.perf_counter() - t, 6))
        for name, (hi, lo) in (("present", present), ("absent", absent)):
            s_host, ids = timed(lambda: g.lookup_nodes(lo, hi))
            tlo, thi = torch.from_numpy(lo.view(np.int64)).to(dev), torch.from_numpy(hi.view(np.int64)).to(dev)
            s_dev, _ = timed(lambda: g.lookup_nodes(tlo, thi))
            out(step="lookup", size=size, path=path, keys=name, n=nq, found=int((ids != 0xFFFFFFFF).sum()),
                host_arrays_s=round(s_host, 6), device_tensors_s=round(s_dev, 6), device_keys_per_s=round(nq / s_dev))
        after = g.stats()
        out(step="lookup", size=size, path=path, counters={n: after[n] - before[n] for n in
                                                            ("lookup_dir_calls", "lookup_index_calls", "lookup_index_builds")})


def step_score(size, args):
    import numpy as np
    g, c = graph_for(size, True)
    k, n_seq, length = c["k"], 100_000, 1000
    rng = np.random.default_rng(11)
    starts = rng.integers(0, c["glen"] - length, n_seq)
    texts = [genome_text(c, int(s), length) for s in starts[:100]]
    # the other sequences come out of one long stretch of the genome, cut at random places: the same kind of text
    stretch = genome_text(c, 0, min(c["glen"], 4_000_000))
    cut = rng.integers(0, len(stretch) - length, n_seq - 100)
    chars = b"".join(texts) + b"".join(stretch[int(a):int(a) + length] for a in cut)
    offsets = np.arange(0, (n_seq + 1) * length, length, dtype=np.uint64)
    for path in ("directory", "index"):
        g.set_option("lookup_index", 1 if path == "index" else 0)
        g.score_sequences(chars[:length], offsets[:2])  # the index, if this path needs one
        best = None
        for _ in range(3):
            t = time.perf_counter()
            scores, miss = g.score_sequences(chars, offsets)
            dt = time.perf_counter() - t
            best = dt if best is None else min(best, dt)
        out(step="score", size=size, path=path, n_seq=n_seq, chars=len(chars), seconds=round(best, 6),
            windows_per_s=round(n_seq * (length - k) / best), complete=int((miss == np.iinfo(np.uint64).max).sum()))
    g.set_option("lookup_index", 0)
    if args.no_host_loop:
        return
    V, E, ect = views_over(g, k)
    t = time.perf_counter()
    len(ect)  # loads the arrays: the host path from here on
    load = time.perf_counter() - t
    t = time.perf_counter()
    host, first = [], True
    for s in texts:
        s = s.decode()
        total = 0
        for i in range(len(s) - k):
            try:
                total += ect[s[i:i + k + 1]]
            except KeyError:
                pass
        host.append(total)
        if first:
            out(step="score", size=size, what="host getScore loop, first sequence (sorts the keys)", seconds=round(time.perf_counter() - t, 3))
            first = False
    dt = time.perf_counter() - t
    same = [int(x) for x in scores[:100]] == host
    out(step="score", size=size, what="host getScore loop over the loaded views", sequences=100, load_arrays_s=round(load, 3),
        seconds=round(dt, 3), windows_per_s=round(100 * (length - k) / dt), equal_to_device=same)
    if not same:
        raise SystemExit("device scores differ from the host loop")


STEPS = {"view": step_view, "lookup": step_lookup, "score": step_score}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="bench,k63")
    ap.add_argument("--steps", default="view,lookup,score")
    ap.add_argument("--pkg", default="", help="py-debruijn_amd of another (built) checkout, for the view step")
    ap.add_argument("--no-host-loop", action="store_true")
    ap.add_argument("--limit", type=int, default=600, help="seconds per step")
    ap.add_argument("--child", nargs=2, metavar=("STEP", "SIZE"))
    args = ap.parse_args()
    if args.child:
        sys.path.insert(0, args.pkg or os.path.join(ROOT, "py-debruijn_amd"))
        import torch
        torch.zeros(1, device="cuda")
        STEPS[args.child[0]](args.child[1], args)
        return 0
    for size in args.sizes.split(","):
        for step in args.steps.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", step, size, "--limit", str(args.limit)]
            if args.pkg:
                cmd += ["--pkg", args.pkg]
            if args.no_host_loop:
                cmd.append("--no-host-loop")
            t = time.perf_counter()
            try:
                rc = subprocess.run(cmd, timeout=args.limit).returncode
            except subprocess.TimeoutExpired:
                out(step=step, size=size, failed=f"no result within {args.limit} s")
                return 1
            if rc != 0:
                out(step=step, size=size, failed=f"exit status {rc}")
                return 1
            out(step=step, size=size, step_wall_s=round(time.perf_counter() - t, 1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
