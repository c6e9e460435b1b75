#!/usr/bin/env python3
"""A/B of the cross-bucket resolver's options in one process, on BASELINE.json configs[1]'s reads:

  direct (default)  option resolve_direct 0 (every query reads and compares its key run) against 1 (the directory entry alone
                    where it names the node) at the flagship size, k = 31 and k = 63, cycled ROUNDS times; per setting
                    ms_succ, ms_count and ms_build_total of a warm build, then one counted build per setting (option
                    resolve_count: the share of queries the entry decided).
  sorted            option resolve_sorted 0 (the askers' bucket order) against 1 (grouped by the 512 level-1 groups of the
                    target); ms_succ covers the grouping.

usage: resolve_ab.py [direct|sorted] [ROUNDS]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "py-debruijn_amd"))
import torch  # noqa: E402

torch.zeros(1, device="cuda")
import _dbg  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "direct"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3


def warm_build(g, k):
    g.build(k)
    g.build(k)
    return g.stats(), g.sizes()


if mode == "sorted":
    for (n, glen, err, k) in ((10000000, 50000000, 0.01, 31), (10000000, 50000000, 0.01, 21), (3000000, 15000000, 0.02, 31)):
        g = _dbg.Graph()
        g.synth_reads(1, glen, n, 150, err)
        for rs in (0, 1, 0, 1):
            g.set_option("resolve_sorted", rs)
            st, sz = warm_build(g, k)
            print(n, k, "resolve_sorted", rs, sz["n_nodes"], st["n_queries"], "succ ms", round(st["ms_succ"], 3), "build ms", round(st["ms_build_total"], 3), flush=True)
        g.close()
else:
    n, glen, err = 10000000, 50000000, 0.01
    for k in (31, 63):
        g = _dbg.Graph()
        g.synth_reads(1, glen, n, 150, err)
        for _ in range(rounds):
            for rd in (0, 1):
                g.set_option("resolve_direct", rd)
                st, sz = warm_build(g, k)
                print(n, k, "resolve_direct", rd, sz["n_nodes"], st["n_queries"], "succ ms", round(st["ms_succ"], 3),
                      "count ms", round(st["ms_count"], 3), "build ms", round(st["ms_build_total"], 3), flush=True)
        g.set_option("resolve_count", 1)
        for rd in (0, 1):
            before = g.stats()
            g.set_option("resolve_direct", rd)
            g.build(k)
            st = g.stats()
            hits, keyed = (st[c] - before[c] for c in ("resolve_direct_hits", "resolve_keyed"))
            print(n, k, "resolve_direct", rd, "counted:", st["n_queries"], "queries,", hits, "direct,", keyed, "keyed, share",
                  round(hits / max(st["n_queries"], 1), 4), "(succ ms with counting", round(st["ms_succ"], 3), ")", flush=True)
        g.close()
