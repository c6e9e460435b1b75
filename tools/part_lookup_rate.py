#!/usr/bin/env python3
"""Rates of the query side of a graph in parts (dbg_part_lookup_nodes_device, dbg_part_score_sequences) beside the same
queries on a single graph of the same reads, at two sizes:

  bench   10 M x 150 bp synthetic reads, k = 31 (BASELINE.json configs[1]) as build_multipass(31, 4) and as build(31)
  k63     1 M x 150 bp, k = 63 (two-word keys), in 4 parts and whole

One child process per size holds both graphs and runs everything in one call:

  lookup   1e7 present and 1e7 absent keys from device tensors through the parts (the kernel routes every key to its part),
           through the single graph's directory and through its sorted index ("lookup_index" 1; the sort that builds the
           index is reported by itself)
  score    score_sequences over 1e5 substrings of the genome of 1 000 characters each, through the parts, the directory and
           the index

Best of 3, the variants alternating inside every repetition; the answers of the variants are compared (the same keys are
found, the same scores come out).

usage: part_lookup_rate.py [--sizes bench,k63] [--passes 4] [--limit SECONDS]
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


def genome_text(start, length):
    import numpy as np
    import synth
    return synth.ALPHABET[synth.genome_codes(SEED, start, length).astype(np.intp)].tobytes()


def best_of(variants, reps=3):
    """variants: name -> fn.  -> (name -> best seconds, name -> last result); the variants alternate inside a repetition."""
    import torch
    best, last = {}, {}
    for _ in range(reps):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            last[name] = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            best[name] = dt if name not in best else min(best[name], dt)
    return best, last


def run_size(size, n_passes):
    import numpy as np
    import torch
    import _dbg
    c = SIZES[size]
    k = c["k"]
    gp, gs = _dbg.Graph(), _dbg.Graph()
    for g in (gp, gs):
        g.synth_reads(SEED, c["glen"], c["n"], READ_LEN, c["err"])
    gp.build_multipass(k, n_passes)
    gs.build(k)
    n_nodes = gs.sizes()["n_nodes"]
    parts = [gp.part_sizes(p)["n_nodes"] for p in range(n_passes)]
    if sum(parts) != n_nodes:
        raise SystemExit(f"the parts hold {sum(parts)} nodes, the single graph {n_nodes}")
    out(step="graphs", size=size, k=k, n_nodes=n_nodes, part_nodes=parts)
    dev = torch.device("cuda", gs.sizes_device())
    nq = 10_000_000
    rng = np.random.default_rng(7)
    rows = gs.gather_nodes(rng.integers(0, n_nodes, nq), what=("keys", "keys_hi"))
    width = 2 * k
    queries = {"present": (rows["keys_hi"], rows["keys"]),
               "absent": (rng.integers(0, 1 << 64, nq, dtype=np.uint64) & np.uint64(((1 << width) - 1) >> 64),
                          rng.integers(0, 1 << 64, nq, dtype=np.uint64) & np.uint64(((1 << width) - 1) & ((1 << 64) - 1)))}
    t = time.perf_counter()
    gs.set_option("lookup_index", 1)
    gs.lookup_nodes(rows["keys"][:1], rows["keys_hi"][:1])
    out(step="lookup", size=size, what="first call through the index (sorts it)", seconds=round(time.perf_counter() - t, 6))
    gp.part_lookup_nodes(rows["keys"][:1], rows["keys_hi"][:1])  # the descriptor table
    before = {**gs.stats(), **{"part_lookup_calls": gp.stats()["part_lookup_calls"]}}

    def single(index, fn):
        def run():
            gs.set_option("lookup_index", index)
            return fn()
        return run

    for name, (hi, lo) in queries.items():
        tlo, thi = torch.from_numpy(lo.view(np.int64)).to(dev), torch.from_numpy(hi.view(np.int64)).to(dev)
        best, last = best_of({"parts": lambda: gp.part_lookup_nodes(tlo, thi),
                              "directory": single(0, lambda: gs.lookup_nodes(tlo, thi)),
                              "index": single(1, lambda: gs.lookup_nodes(tlo, thi))})
        found = {"parts": int((last["parts"][1] != -1).sum()), "directory": int((last["directory"] != -1).sum()),
                 "index": int((last["index"] != -1).sum())}
        if len(set(found.values())) != 1 or (name == "present" and found["parts"] != nq):
            raise SystemExit(f"the variants disagree on the {name} keys: {found}")
        out(step="lookup", size=size, keys=name, n=nq, found=found["parts"],
            seconds={v: round(s, 6) for v, s in best.items()}, keys_per_s={v: round(nq / s) for v, s in best.items()})
    # score_sequences: 1e5 substrings of the genome, 1 000 characters each
    n_seq, length = 100_000, 1000
    stretch = genome_text(0, min(c["glen"], 4_000_000))
    cut = rng.integers(0, len(stretch) - length, n_seq)
    chars = b"".join(stretch[int(a):int(a) + length] for a in cut)
    offsets = np.arange(0, (n_seq + 1) * length, length, dtype=np.uint64)
    best, last = best_of({"parts": lambda: gp.part_score_sequences(chars, offsets),
                          "directory": single(0, lambda: gs.score_sequences(chars, offsets)),
                          "index": single(1, lambda: gs.score_sequences(chars, offsets))})
    for v in ("directory", "index"):
        if not (np.array_equal(last["parts"][0], last[v][0]) and np.array_equal(last["parts"][1], last[v][1])):
            raise SystemExit(f"the scores through the parts differ from those through the single graph's {v}")
    out(step="score", size=size, n_seq=n_seq, chars=len(chars), complete=int((last["parts"][1] == np.iinfo(np.uint64).max).sum()),
        seconds={v: round(s, 6) for v, s in best.items()},
        windows_per_s={v: round(n_seq * (length - k) / s) for v, s in best.items()})
    gs.set_option("lookup_index", 0)
    after = {**gs.stats(), **{"part_lookup_calls": gp.stats()["part_lookup_calls"]}}
    out(step="counters", size=size, calls={n: after[n] - before[n] for n in
                                           ("part_lookup_calls", "lookup_dir_calls", "lookup_index_calls", "lookup_index_builds")})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="bench,k63")
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--limit", type=int, default=600, help="seconds per size")
    ap.add_argument("--child", metavar="SIZE")
    args = ap.parse_args()
    if args.child:
        sys.path.insert(0, os.path.join(ROOT, "py-debruijn_amd"))
        import torch
        torch.zeros(1, device="cuda")
        run_size(args.child, args.passes)
        return 0
    for size in args.sizes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", size, "--passes", str(args.passes)]
        t = time.perf_counter()
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            out(size=size, failed=f"no result within {args.limit} s")
            return 1
        if rc != 0:
            out(size=size, failed=f"exit status {rc}")
            return 1
        out(size=size, wall_s=round(time.perf_counter() - t, 1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
