#!/usr/bin/env python3
"""Time of the both-strands pass (dbg_add_revcomp) on the configs[1] reads (GPU box): N x 150 bp synthetic
reads made on the device, 1.5 GB of bases at 10 M reads.

In every round, in one process:
  revcomp  add_revcomp on the forward reads: N bytes read, 2N written -- host clock around the call (allocations, the
           start bitmap and the synchronise included) and the call's own ms_kernel (events around its kernels)
  split    split_reads on the same reads, which have nothing to cut: one read of the N bytes, nothing written
  copy     a device-to-device hipMemcpyAsync of 2N bytes through torch (2N read, 2N written), by events and by host clock
Each is the best of --reps, all of them listed.  Then the graph at k = 31 of the forward reads and of both strands: build
time (host clock) and node counts.  One JSON line on stdout.

    python tools/revcomp.py [--reads 10e6] [--reps 5] [--k 31] [--no-graph]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "py-debruijn_amd"))
import _dbg  # noqa: E402

L = 150


def ms(fn):
    t = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t) * 1e3, r


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=float, default=10e6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--no-graph", action="store_true")
    args = ap.parse_args()
    n = int(args.reads)
    nb = n * L
    g = _dbg.Graph()
    src = torch.empty(2 * nb, dtype=torch.uint8, device="cuda").random_(65, 85)
    dst = torch.empty_like(src)
    torch.cuda.synchronize()
    res = {"tool": "revcomp", "reads": n, "read_len": L, "n_bytes": nb, "reps": args.reps,
           "revcomp_host_ms": [], "revcomp_kernel_ms": [], "split_clean_host_ms": [], "copy_2n_event_ms": [], "copy_2n_host_ms": []}
    st = None
    for _ in range(args.reps):
        g.synth_reads(1, n * 5, n, L, 0.01)
        g.reads_checksum()  # ends in a synchronise: the reads are there
        t, sp = ms(lambda: g.split_reads())
        assert sp["changed"] == 0
        res["split_clean_host_ms"].append(round(t, 3))
        t, st = ms(lambda: g.add_revcomp())
        res["revcomp_host_ms"].append(round(t, 3))
        res["revcomp_kernel_ms"].append(round(st["ms_kernel"], 3))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        dst.copy_(src, non_blocking=True)
        b.record()
        torch.cuda.synchronize()
        res["copy_2n_host_ms"].append(round((time.perf_counter() - t0) * 1e3, 3))
        res["copy_2n_event_ms"].append(round(a.elapsed_time(b), 3))
    del src, dst
    torch.cuda.empty_cache()
    for f in ("revcomp_host_ms", "revcomp_kernel_ms", "split_clean_host_ms", "copy_2n_event_ms", "copy_2n_host_ms"):
        res[f.replace("_ms", "_best_ms")] = min(res[f])
    res["kernel_over_copy_2n"] = round(res["revcomp_kernel_best_ms"] / res["copy_2n_event_best_ms"], 3)
    res["kernel_gb_per_s"] = round(3 * nb / res["revcomp_kernel_best_ms"] / 1e6, 1)  # N read + 2N written
    res["copy_2n_gb_per_s"] = round(4 * nb / res["copy_2n_event_best_ms"] / 1e6, 1)  # 2N read + 2N written
    res.update({f: st[f] for f in ("n_reads_out", "n_bytes_out", "n_other_bytes", "n_palindromes", "peak_extra_device_bytes")})
    if not args.no_graph:
        res["k"] = args.k
        for name, both in (("forward", False), ("both", True)):
            times = []
            for _ in range(2):  # the first build of a size also allocates its arenas
                g.synth_reads(1, n * 5, n, L, 0.01)
                if both:
                    g.add_revcomp()
                g.reads_checksum()
                times.append(round(ms(lambda: g.build(args.k))[0], 1))
            res.update({name + "_build_ms": times, name + "_build_best_ms": min(times), name + "_nodes": g.sizes()["n_nodes"]})
    g.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
