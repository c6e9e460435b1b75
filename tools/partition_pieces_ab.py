#!/usr/bin/env python3
"""A/B of the pieces of the first half of the build -- the small-fan-out scatter of level 1, the super-chunk length, the
extraction grid -- in ONE process: every setting is a build of the library (csrc/build.sh with DBG_OUT into a file of its
own, from sources with the piece in or out) plus an extract_grid value, each library is loaded beside the others, and the
settings are visited in turn, twice.  Every library brings a handle and an arena of its own, and where an arena lies moves a
partition time by tenths of a millisecond: compare the visits of ONE library (the grids) closely, libraries with each other
only roughly, and settle those with bench.py in processes of their own (DBG_LIB).  To load several libraries the tool sets
_dbg.LIB_PATH and clears _dbg's cached library before each load; nothing else may do that.

    tools/partition_pieces_ab.py label=path/to/lib.so[:extract_grid] ...

Reads as in tools/presplit_ab.py: BASELINE.json configs[1]'s at k = 31 and k = 21, and 3 M reads at k = 31.  A visit is two
builds; the second one's extraction, partition and build times are printed."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "py-debruijn_amd"))
import torch  # noqa: E402

torch.zeros(1, device="cuda")
import _dbg  # noqa: E402

# a library from before the ms_scatter_* counters must load too
_dbg.COUNTERS = tuple(c for c in _dbg.COUNTERS if not c.startswith("ms_scatter_"))
VISITS = 2


def graph_on(path):
    """A handle of the library at `path` (its own copy of the code: another file, another load)."""
    _dbg._lib = None
    _dbg.LIB_PATH = path
    return _dbg.Graph()


settings = []
for arg in sys.argv[1:]:
    label, rest = arg.split("=", 1)
    path, _, grid = rest.partition(":")
    settings.append((label, os.path.abspath(path), int(grid) if grid else None))

for (n, glen, err, k) in ((10000000, 50000000, 0.01, 31), (10000000, 50000000, 0.01, 21), (3000000, 15000000, 0.02, 31)):
    graphs = {}
    for label, path, grid in settings:
        if path not in graphs:
            graphs[path] = graph_on(path)
            graphs[path].synth_reads(1, glen, n, 150, err)
            graphs[path].build(k)  # the arena
    for visit in range(VISITS):
        for label, path, grid in settings:
            g = graphs[path]
            if grid is not None:
                g.set_option("extract_grid", grid)
            g.build(k)
            g.build(k)
            st, sz = g.stats(), g.sizes()
            print(n, k, label, "visit", visit, sz["n_nodes"], st["n_records"], st["n_buckets"], "fallbacks",
                  st["extract_presplit_fallbacks"], "extract ms", round(st["ms_extract"], 3), "partition ms",
                  round(st["ms_partition"], 3), "build ms", round(st["ms_build_total"], 3), flush=True)
    for g in graphs.values():
        g.close()
