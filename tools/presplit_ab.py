#!/usr/bin/env python3
"""A/B of the pre-split extraction (option extract_presplit: 0 = one segment per extraction workgroup, f0 = the records of a
workgroup split by the top f0 bits of the bucket hash and level 1 of the multisplit run per group) on BASELINE.json
configs[1]'s reads, at k = 21 and on 3 M reads: extraction, partition and build time per setting, one process."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "py-debruijn_amd"))
import torch  # noqa: E402

torch.zeros(1, device="cuda")
import _dbg  # noqa: E402

for (n, glen, err, k) in ((10000000, 50000000, 0.01, 31), (10000000, 50000000, 0.01, 21), (3000000, 15000000, 0.02, 31)):
    g = _dbg.Graph()
    g.synth_reads(1, glen, n, 150, err)
    for f0 in (0, 3, 4, 5, 6) * 2:
        g.set_option("extract_presplit", f0)
        g.build(k)
        g.build(k)
        st, sz = g.stats(), g.sizes()
        print(n, k, "extract_presplit", f0, sz["n_nodes"], st["n_records"], st["n_buckets"], "fallbacks", st["extract_presplit_fallbacks"],
              "extract ms", round(st["ms_extract"], 3), "partition ms", round(st["ms_partition"], 3),
              "build ms", round(st["ms_build_total"], 3), flush=True)
    g.close()
